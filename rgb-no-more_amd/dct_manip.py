"""Drop-in for the reference's `dct_manip` extension module on this path: `read_coefficients(path)` with the same
return contract (dct_manip/dct_manip.cpp:152-178), implemented by the host C library librgbnm_reader.so
(csrc/reader.c, include/rgbnm_reader.h) through ctypes -- no libtorch / pybind11 in the native part.

    dim, quant, Y, CbCr = dct_manip.read_coefficients("img.jpg")
    dim int32 (C,2); quant int16 (C,8,8); Y int16 (1,Hb,Wb,8,8); CbCr int16 (2,Hb/2,Wb/2,8,8) or None (grayscale)

`read_coefficients_batch` decodes many same-shaped files with a pthread pool into pinned batch tensors ready for one
H2D copy (replaces per-sample tensors + default collate, datasets.py:274-297,542-546).

`quantize_at_quality` and `decode_coeff` (dct_manip.cpp:315-375, 485-576) run on DEVICE tensors, one HIP launch per call
(csrc/pixel_dct.hip), for one image or a batch; there is no CPU fallback.

`write_coefficients` (dct_manip.cpp:265-313) writes the reference's file byte for byte, Huffman-encoded on the device
(csrc/jpeg_encode.hip); `encode_jpeg_batch` / `write_coefficients_batch` are its batched forms, optionally with restart markers.
"""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librgbnm_reader.so")
_lib = None
_ERRLEN = 512


class libjpeg_exception(Exception):
    """mirrors dct_manip.cpp:24-41 (libjpeg's formatted message)."""


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"host reader missing: {LIB_PATH} (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        L.rgbnm_reader_abi_version.restype = C.c_int
        L.rgbnm_jpeg_info.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
        L.rgbnm_jpeg_info_mem.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_int]
        L.rgbnm_read_coefficients.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        L.rgbnm_read_coefficients_mem.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_char_p, C.c_int]
        L.rgbnm_read_coefficients_batch.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rgbnm_read_coefficients_batch_crop.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
        for f in ("rgbnm_jpeg_info", "rgbnm_jpeg_info_mem", "rgbnm_read_coefficients", "rgbnm_read_coefficients_mem",
                  "rgbnm_read_coefficients_batch", "rgbnm_read_coefficients_batch_crop"):
            getattr(L, f).restype = C.c_int
        _lib = L
    return _lib


def _raise(rc, err):
    msg = err.value.decode(errors="replace")
    if rc == -1:
        raise RuntimeError(msg)                      # "Unable to open file for reading: ..."
    if rc == -2:
        raise libjpeg_exception(msg)
    raise RuntimeError(f"read_coefficients failed ({rc}) {msg}")


def _read(path=None, data=None):
    L = lib()
    err = C.create_string_buffer(_ERRLEN)
    info = (C.c_int32 * 17)()
    if data is None:
        p = os.fsencode(path)
        rc = L.rgbnm_jpeg_info(p, info, err, _ERRLEN)
    else:
        rc = L.rgbnm_jpeg_info_mem(data, len(data), info, err, _ERRLEN)
    if rc:
        _raise(rc, err)
    nc = info[0]
    hb, wb = info[1], info[2]
    if nc not in (1, 3):
        raise libjpeg_exception(f"unsupported JPEG: {nc} components (the DCT path reads grayscale or YCbCr files)")
    dim = torch.empty((nc, 2), dtype=torch.int32)
    quant = torch.empty((nc, 8, 8), dtype=torch.int16)
    Y = torch.empty((1, hb, wb, 8, 8), dtype=torch.int16)
    CbCr = None
    if nc > 1:
        CbCr = torch.empty((2, info[5], info[6], 8, 8), dtype=torch.int16)
    cptr = CbCr.data_ptr() if CbCr is not None else None
    if data is None:
        rc = L.rgbnm_read_coefficients(p, dim.data_ptr(), quant.data_ptr(), Y.data_ptr(), cptr, err, _ERRLEN)
    else:
        rc = L.rgbnm_read_coefficients_mem(data, len(data), dim.data_ptr(), quant.data_ptr(), Y.data_ptr(), cptr, err, _ERRLEN)
    if rc:
        _raise(rc, err)
    return dim, quant, Y, CbCr


def read_coefficients(path: str):
    """(dim, quant, Y, CbCr|None) -- reference: dct_manip.read_coefficients (dct_manip.cpp:152-178)."""
    return _read(path=path)


def read_coefficients_bytes(data: bytes):
    """Same, from an in-memory JPEG."""
    return _read(data=bytes(data))


def default_threads():
    """Decoder threads worth starting: the CPUs this process may actually use (cgroup quota / affinity), not os.cpu_count()
    (the GPU box shows 256 hardware threads and grants 16: 256 decoder threads ran 35 % slower than 16)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    return n


def alloc_batch(n, grid=(64, 64), pin_memory=True):
    """Reusable (pinned) staging buffers for read_coefficients_batch(out=...): allocating pinned memory per batch costs
    more than decoding it."""
    hb, wb = grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    kw = dict(dtype=torch.int16, pin_memory=pin_memory)
    return (torch.empty((n, 1, hb, wb, 8, 8), **kw), torch.empty((n, 2, hbc, wbc, 8, 8), **kw),
            torch.empty((n, 3, 8, 8), **kw))


def read_coefficients_batch(paths, threads=8, grid=(64, 64), pin_memory=False, out=None):
    """Decode len(paths) JPEGs of one coefficient grid (default 512x512 4:2:0 -> 64x64 luma blocks) in parallel.
    Returns Y (B,1,Hb,Wb,8,8), CbCr (B,2,Hb/2,Wb/2,8,8), quant (B,3,8,8) int16 CPU tensors (optionally pinned);
    out = buffers from alloc_batch() to decode into (ring of staging buffers)."""
    L = lib()
    n = len(paths)
    hb, wb = grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    if out is None:
        out = alloc_batch(n, grid, pin_memory)
    Y, CbCr, quant = out
    if tuple(Y.shape) != (n, 1, hb, wb, 8, 8) or tuple(CbCr.shape) != (n, 2, hbc, wbc, 8, 8) or \
            tuple(quant.shape) != (n, 3, 8, 8) or any(t.dtype != torch.int16 or not t.is_contiguous() for t in out):
        raise ValueError("out buffers do not match the batch (use alloc_batch)")
    status = torch.zeros(n, dtype=torch.int32)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    bad = L.rgbnm_read_coefficients_batch(arr, n, int(threads), hb, wb, hbc, wbc, Y.data_ptr(), CbCr.data_ptr(),
                                          quant.data_ptr(), status.data_ptr())
    if bad:
        i = int((status != 0).nonzero()[0])
        code = int(status[i])
        if code == -1:
            raise RuntimeError(f"Unable to open file for reading: {paths[i]}")
        raise libjpeg_exception(f"{paths[i]}: reader error {code} ({bad} of {n} files failed)")
    return Y, CbCr, quant


def _raise_batch(paths, status, bad):
    i = int((status != 0).nonzero()[0])
    code = int(status[i])
    if code == -1:
        raise RuntimeError(f"Unable to open file for reading: {paths[i]}")
    raise libjpeg_exception(f"{paths[i]}: reader error {code} ({bad} of {len(paths)} files failed)")


def alloc_packed(n, grid=(64, 64), pin_memory=True):
    """Staging buffers for read_coefficients_batch_crop(out=...): flat int16 Y / CbCr buffers sized for n WHOLE grids (a
    batch of crops never needs more), quant (n,3,8,8)."""
    hb, wb = grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    kw = dict(dtype=torch.int16, pin_memory=pin_memory)
    return (torch.empty(n * hb * wb * 64, **kw), torch.empty(n * 2 * hbc * wbc * 64, **kw), torch.empty((n, 3, 8, 8), **kw))


def packed_offsets(boxes):
    """boxes int (n,4) = (top, left, height, width) in luma blocks -> element offsets of every image's crop in the flat Y /
    CbCr buffers (running sums of the box sizes) and the totals: (y_off int64 (n,), c_off int64 (n,), n_y, n_c)."""
    b = torch.as_tensor(boxes, dtype=torch.int64)
    ysz = b[:, 2] * b[:, 3] * 64
    csz = 2 * (b[:, 2] // 2) * (b[:, 3] // 2) * 64
    y_off = torch.cumsum(ysz, 0) - ysz
    c_off = torch.cumsum(csz, 0) - csz
    return y_off.contiguous(), c_off.contiguous(), int(ysz.sum()), int(csz.sum())


def read_coefficients_batch_crop(paths, boxes, threads=8, grid=(64, 64), pin_memory=False, out=None):
    """Decode len(paths) same-grid JPEGs and keep only each file's crop box (luma blocks (top, left, height, width), all
    even; the chroma box is the luma box halved), packed back to back: returns (Ypacked, Cpacked, quant, y_off, c_off) --
    flat int16 buffers trimmed to the used length, image i's luma crop [h][w][8][8] at Ypacked[y_off[i]:], its chroma crop
    [2][h/2][w/2][8][8] at Cpacked[c_off[i]:].  What crosses PCIe afterwards is the crop, not the 64 x 64 grid."""
    L = lib()
    n = len(paths)
    hb, wb = grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    bx = torch.as_tensor(boxes, dtype=torch.int32).contiguous()
    if tuple(bx.shape) != (n, 4):
        raise ValueError("boxes must be (len(paths), 4)")
    y_off, c_off, ny, ncc = packed_offsets(bx)
    if out is None:
        out = alloc_packed(n, grid, pin_memory)
    Yp, Cp, quant = out
    if Yp.numel() < ny or Cp.numel() < ncc or tuple(quant.shape)[1:] != (3, 8, 8) or quant.shape[0] < n or \
            any(t.dtype != torch.int16 or not t.is_contiguous() for t in out):
        raise ValueError("out buffers too small for this batch (use alloc_packed)")
    status = torch.zeros(n, dtype=torch.int32)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    bad = L.rgbnm_read_coefficients_batch_crop(arr, n, int(threads), hb, wb, hbc, wbc, bx.data_ptr(), y_off.data_ptr(),
                                               c_off.data_ptr(), Yp.data_ptr(), Cp.data_ptr(), quant.data_ptr(),
                                               status.data_ptr())
    if bad:
        if int(status[(status != 0).nonzero()[0]]) == -3:
            raise ValueError("crop box outside the coefficient grid (or not even)")
        _raise_batch(paths, status, bad)
    return Yp[:ny], Cp[:ncc], quant[:n], y_off, c_off


# ---- entropy decode on the device (csrc/jpeg_scan.h, jpeg_walk.h, jpeg_decode.hip; include/rgbnm.h) -------------------------------
_MSGLEN = 128


class JpegBatchPlan:
    """The buffers rgbnm_jpeg_prepare fills (include/rgbnm.h, rgbnm_jpeg_plan) as CPU tensors -- pinned when asked, so that each is
    one asynchronous H2D copy -- and, after prepare_jpeg_batch, the counts, the per-file status (0, or a negative RGBNM_JPEG_E* code)
    and message.  Sized once for batches of up to n files and re-used (a ring of them in the loader):
        stream uint8 [stream_cap] | runs int32 [runs_cap, 8] | images int32 [n, 48] | tables uint8 [tables_cap, 1440]
        quant int16 [n, 3, 8, 8] | status int32 [n]"""

    def __init__(self, n, grid=(64, 64), stream_cap=None, runs_cap=None, tables_cap=None, pin_memory=False):
        hb, wb = grid
        hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
        if stream_cap is None:                       # 192 KB per 512 x 512 file (quality 90 on a noisy image: 98 KB), one run per MCU row ...
            stream_cap = n * max(4096, 48 * hb * wb)
        if runs_cap is None:                         # ... up to one run per 4:2:0 MCU
            runs_cap = n * max(64, hbc * wbc)
        if tables_cap is None:
            tables_cap = min(65535, 4 + 6 * n)
        kw = dict(pin_memory=pin_memory)
        self.capacity, self.grid = int(n), (hb, wb)
        self.stream = torch.empty(int(stream_cap) + 8 * int(runs_cap), dtype=torch.uint8, **kw)
        self.runs = torch.empty((int(runs_cap), 8), dtype=torch.int32, **kw)
        self.images = torch.empty((n, 48), dtype=torch.int32, **kw)
        self.tables = torch.empty((int(tables_cap), 1440), dtype=torch.uint8, **kw)
        self.quant = torch.empty((n, 3, 8, 8), dtype=torch.int16, **kw)
        self.status = torch.zeros(n, dtype=torch.int32, **kw)
        self._msg = C.create_string_buffer(n * _MSGLEN)
        self.n = self.nruns = self.ntables = self.stream_bytes = self.nbad = 0
        self.names, self.messages = [], []

    def buffers(self):
        """The used prefixes: what crosses PCIe."""
        return (self.stream[:self.stream_bytes], self.runs[:self.nruns], self.images[:self.n], self.tables[:self.ntables],
                self.quant[:self.n], self.status[:self.n])

    def h2d_bytes(self):
        return sum(t.numel() * t.element_size() for t in self.buffers())


def _read_file(d):
    try:
        with open(d, "rb") as fh:
            return fh.read()
    except OSError:
        raise RuntimeError(f"Unable to open file for reading: {d}") from None


def _jpeg_bytes(datas):
    """(file contents, names) of a list of bytes or paths."""
    isb = [isinstance(d, (bytes, bytearray, memoryview)) for d in datas]
    names = [f"<bytes #{k}>" if b else os.fspath(d) for k, (d, b) in enumerate(zip(datas, isb))]
    return [bytes(d) if b else _read_file(d) for d, b in zip(datas, isb)], names


def prepare_jpeg_batch(datas, grid=(64, 64), out=None, threads=1, pin_memory=False):
    """Host half of the device decode; needs no GPU.  datas: JPEG files as bytes or paths.  Finds the independent bit streams of
    every file -- marker parse, un-stuffing, split at the restart markers; no Huffman decode -- and returns a JpegBatchPlan (out:
    one to fill again) whose buffers decode_jpeg_batch ships and walks.  A file the device cannot decode (progressive, another
    grid, damaged, ...) gets a negative plan.status[i] and plan.messages[i]; the other files are not affected."""
    from . import lib as L
    datas, names = _jpeg_bytes(datas)
    n = len(datas)
    if n == 0:
        raise ValueError("no files")
    hb, wb = grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    if out is None:
        total = sum(len(d) for d in datas)
        out = JpegBatchPlan(n, grid, stream_cap=total + 4 * n, runs_cap=sum(min(hb * wb, len(d) // 2 + 1) for d in datas),
                            pin_memory=pin_memory)
    if n > out.capacity or tuple(out.grid) != (hb, wb):
        raise ValueError("plan buffers do not match the batch (JpegBatchPlan(n, grid))")
    p = L.JpegPlan(stream=out.stream.data_ptr(), stream_cap=out.stream.numel(), runs=out.runs.data_ptr(), images=out.images.data_ptr(),
                   tables=out.tables.data_ptr(), quant=out.quant.data_ptr(), messages=C.addressof(out._msg),
                   runs_cap=out.runs.shape[0], tables_cap=out.tables.shape[0], message_len=_MSGLEN, threads=int(threads))
    bufs = (C.c_char_p * n)(*datas)
    lens = (C.c_size_t * n)(*[len(d) for d in datas])
    rc = L.lib().rgbnm_jpeg_prepare(bufs, lens, n, hb, wb, hbc, wbc, C.byref(p))
    if rc < 0:
        L.check(rc, "jpeg_prepare")
    out.n, out.nruns, out.ntables, out.stream_bytes, out.nbad = n, p.nruns, p.ntables, p.stream_bytes, p.nbad
    out.status[:n] = out.images[:n, 4]
    out.names = names
    out.messages = [out._msg.raw[i * _MSGLEN:(i + 1) * _MSGLEN].split(b"\0", 1)[0].decode(errors="replace") for i in range(n)]
    return out


def alloc_jpeg_out(n, grid=(64, 64), device="cuda"):
    """Device tensors for decode_jpeg_batch(out=...): (Y, CbCr, quant, status)."""
    hb, wb = grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    kw = dict(dtype=torch.int16, device=device)
    return (torch.empty((n, 1, hb, wb, 8, 8), **kw), torch.empty((n, 2, hbc, wbc, 8, 8), **kw), torch.empty((n, 3, 8, 8), **kw),
            torch.empty(n, dtype=torch.int32, device=device))


def upload_jpeg_plan(plan, device):
    """One asynchronous H2D copy per plan buffer on the current stream: (stream, runs, images, tables, quant, status) on the device."""
    return tuple(t.to(device, non_blocking=True) for t in plan.buffers())


# The split decode's defaults (csrc/jpeg_split.h; DESIGN.md 7 has the sweep behind them)
JPEG_SPLIT_SEG_BITS = 2048
JPEG_SPLIT_ROUNDS = 16


def jpeg_split_scratch(plan, seg_bits=None, device="cuda"):
    """uint8 device tensor for launch_jpeg_decode(split=True, scratch=...) on this plan (or any with no more stream bytes and runs)."""
    from . import lib as L
    nbytes = L.lib().rgbnm_jpeg_split_scratch_bytes(plan.stream_bytes, plan.nruns, JPEG_SPLIT_SEG_BITS if seg_bits is None else int(seg_bits))
    if nbytes == 0:
        raise L.RgbnmError("seg_bits must be a multiple of 32 in 128..65536")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def alloc_jpeg_packed(n, grid=(64, 64), device="cuda"):
    """Device tensors for decode_jpeg_batch(boxes=..., out=...): (Ypacked, Cpacked, quant, status), the flat buffers sized for n
    WHOLE grids (a batch of crops never needs more)."""
    hb, wb = grid
    kw = dict(dtype=torch.int16, device=device)
    return (torch.empty(n * hb * wb * 64, **kw), torch.empty(n * 2 * ((hb + 1) // 2) * ((wb + 1) // 2) * 64, **kw),
            torch.empty((n, 3, 8, 8), **kw), torch.empty(n, dtype=torch.int32, device=device))


def _check_boxes(boxes, n, grid):
    """boxes as an int32 CPU (n, 4) tensor; the host crop reader's ValueError for a box it would refuse."""
    bx = torch.as_tensor(boxes).to(device="cpu", dtype=torch.int32).contiguous()
    if tuple(bx.shape) != (n, 4):
        raise ValueError("boxes must be (len(paths), 4)")
    hb, wb = grid
    if bool((bx < 0).any()) or bool((bx[:, 2:] <= 0).any()) or bool((bx & 1).any()) or bool((bx[:, 0] + bx[:, 2] > hb).any()) or \
            bool((bx[:, 1] + bx[:, 3] > wb).any()):
        raise ValueError("crop box outside the coefficient grid (or not even)")
    return bx


def launch_jpeg_decode(plan, dev, out, split=False, seg_bits=None, rounds=None, path=None, scratch=None, boxes=None, packed_out=None,
                       walked=None):
    """The decode launch alone (no copy, no sync: capturable).  dev: upload_jpeg_plan's tensors; out: (Y, CbCr, quant,
    status) device tensors (alloc_jpeg_out); quant and status must already hold the plan's (decode_jpeg_batch copies them).
    split=True: rgbnm_jpeg_decode_batch_split instead -- long runs cut into segments of seg_bits bits, one lane each, `rounds` sync
    launches (defaults JPEG_SPLIT_SEG_BITS / JPEG_SPLIT_ROUNDS); the same bits in `out`.  path: int32 [n] device tensor that receives
    0 (no run split) / 1 (split) / 2 (split, then decoded by the one-lane walk) per file, scratch: jpeg_split_scratch's tensor; each
    is taken from the caching allocator when None.  Returns path (None without split).
    boxes (needs split=False): rgbnm_jpeg_decode_batch_crop instead -- only each file's crop box is walked for and stored.  boxes: int
    (n, 4) array or tensor, (top, left, height, width) in luma blocks, all even; a CPU one is uploaded here (a copy: not capturable),
    an int32 device tensor is used in place.  packed_out = (y_off, c_off, y_elems, c_elems): int64 [n] DEVICE tensors with the element
    offsets of every file's crops in out[0] / out[1], which are then FLAT int16 buffers (alloc_jpeg_packed) of which the first y_elems /
    c_elems elements may be written; None: packed_offsets(boxes), uploaded here.  walked: uint32-sized (int32) [plan.nruns] device
    tensor that receives the MCUs each run's lane walked (0: skipped), or None.  The device checks every box and offset again: a bad one
    gives that file the status RGBNM_JPEG_EBOX and writes nothing of it.  Returns (y_off, c_off) on the device."""
    from . import lib as L
    Y, CbCr, _, status = out
    hb, wb = plan.grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    n = plan.n

    def device_plan():                       # after require_cuda(*dev[:4]): a bad `dev` raises there
        return L.JpegDevicePlan(stream=dev[0].data_ptr(), stream_bytes=plan.stream_bytes, runs=dev[1].data_ptr(), images=dev[2].data_ptr(),
                                tables=dev[3].data_ptr(), nruns=plan.nruns, ntables=plan.ntables)

    if boxes is not None:
        if split:
            raise ValueError("boxes need split=False: the split decode's scout and sync passes must see the whole run whatever the box "
                             "(the split decode for boxes is decode_jpeg_batch_split_crop / launch_jpeg_split_crop)")
        if seg_bits is not None or rounds is not None or path is not None or scratch is not None:
            raise ValueError("seg_bits, rounds, path and scratch belong to split=True")
        L.require_cuda(Y, CbCr, status, *dev[:4])
        with torch.cuda.device(Y.device):
            if not (torch.is_tensor(boxes) and boxes.is_cuda):
                if packed_out is None:
                    y_off, c_off, ny, ncc = packed_offsets(_check_boxes(boxes, n, plan.grid))
                    packed_out = (y_off.to(Y.device, non_blocking=True), c_off.to(Y.device, non_blocking=True), ny, ncc)
                boxes = torch.as_tensor(boxes).to(device="cpu", dtype=torch.int32).contiguous().to(Y.device, non_blocking=True)
            elif packed_out is None:
                raise ValueError("device boxes need packed_out=(y_off, c_off, y_elems, c_elems)")
            y_off, c_off, ny, ncc = packed_out
            L.require_cuda(boxes, y_off, c_off)
            if boxes.dtype != torch.int32 or tuple(boxes.shape) != (n, 4) or not boxes.is_contiguous():
                raise L.RgbnmError("boxes must be int32 (n, 4)")
            if any(t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous() for t in (y_off, c_off)):
                raise L.RgbnmError("y_off and c_off must be int64 [n]")
            if Y.dim() != 1 or CbCr.dim() != 1 or Y.dtype != torch.int16 or CbCr.dtype != torch.int16 or not Y.is_contiguous() \
                    or not CbCr.is_contiguous() or int(ny) > Y.numel() or int(ncc) > CbCr.numel() or status.numel() != n \
                    or status.dtype != torch.int32:
                raise L.RgbnmError("out tensors do not match the boxes (alloc_jpeg_packed)")
            if walked is not None:
                L.require_cuda(walked)
                if walked.dtype != torch.int32 or walked.numel() < plan.nruns or not walked.is_contiguous():
                    raise L.RgbnmError("walked must be int32 [plan.nruns]")
            dp = device_plan()
            L.check(L.lib().rgbnm_jpeg_decode_batch_crop(C.byref(dp), n, hb, wb, hbc, wbc, boxes.data_ptr(),
                                                         y_off.data_ptr(), c_off.data_ptr(), Y.data_ptr(), int(ny), CbCr.data_ptr(), int(ncc),
                                                         status.data_ptr(), walked.data_ptr() if walked is not None else None, L.stream()),
                    "jpeg_decode_batch_crop")
        return y_off, c_off
    if packed_out is not None or walked is not None:
        raise ValueError("packed_out and walked belong to boxes")
    L.require_cuda(Y, CbCr, status, *dev[:4])
    if tuple(Y.shape) != (n, 1, hb, wb, 8, 8) or tuple(CbCr.shape) != (n, 2, hbc, wbc, 8, 8) or status.numel() != n \
            or Y.dtype != torch.int16 or CbCr.dtype != torch.int16 or status.dtype != torch.int32:
        raise L.RgbnmError("out tensors do not match the plan (alloc_jpeg_out)")
    dp = device_plan()
    if not split:
        if seg_bits is not None or rounds is not None or path is not None or scratch is not None:
            raise ValueError("seg_bits, rounds, path and scratch belong to split=True")
        with torch.cuda.device(Y.device):
            L.check(L.lib().rgbnm_jpeg_decode_batch(C.byref(dp), n, hb, wb, hbc, wbc, Y.data_ptr(), CbCr.data_ptr(),
                                                    status.data_ptr(), L.stream()), "jpeg_decode_batch")
        return None
    seg_bits = JPEG_SPLIT_SEG_BITS if seg_bits is None else int(seg_bits)
    rounds = JPEG_SPLIT_ROUNDS if rounds is None else int(rounds)
    with torch.cuda.device(Y.device):
        if scratch is None:
            scratch = jpeg_split_scratch(plan, seg_bits, Y.device)
        if path is None:
            path = torch.empty(n, dtype=torch.int32, device=Y.device)
        L.require_cuda(path, scratch)
        if path.dtype != torch.int32 or path.numel() != n or not path.is_contiguous() or scratch.dtype != torch.uint8 \
                or not scratch.is_contiguous():
            raise L.RgbnmError("path must be int32 [n], scratch uint8 (jpeg_split_scratch)")
        L.check(L.lib().rgbnm_jpeg_decode_batch_split(C.byref(dp), n, hb, wb, hbc, wbc, Y.data_ptr(), CbCr.data_ptr(),
                                                      status.data_ptr(), path.data_ptr(), scratch.data_ptr(), scratch.numel(), seg_bits,
                                                      rounds, L.stream()), "jpeg_decode_batch_split")
    return path


def decode_jpeg_batch(plan, device="cuda", out=None, split=False, seg_bits=None, rounds=None, return_path=False, boxes=None):
    """Device half: one H2D copy per plan buffer on the current stream, then ONE launch that walks every run with one lane (there is
    no CPU fallback).  Returns (Y, CbCr, quant, status) on the device: the int16 tensors of read_coefficients_batch, bit for bit, and
    int32 status per file -- the plan's host status, lowered to a negative code where the walk met an error in the stream (the file's
    blocks not yet written are then zeros).  Files with a negative HOST status are not written at all.  No host sync.
    split=True: the split decode instead (launch_jpeg_decode), for files without restart markers; the same four tensors, and with
    return_path=True a fifth, the int32 path per file.
    boxes (int (n, 4), luma blocks, even; needs split=False): the crop decode instead (launch_jpeg_decode) -- returns (Ypacked,
    Cpacked, quant, status, y_off, c_off): the flat tensors of read_coefficients_batch_crop trimmed to packed_offsets(boxes)' totals,
    y_off / c_off int64 on the device: what custom_transforms.apply_packed(..., y_off=, c_off=, grid=) takes.  out: alloc_jpeg_packed's.
    A status of 0 then says nothing about the stream bytes behind the last MCU a file's box needed."""
    if return_path and not split:
        raise ValueError("return_path belongs to split=True")
    n = plan.n
    if boxes is not None:
        if split:
            raise ValueError("boxes need split=False: the split decode's scout and sync passes must see the whole run whatever the box "
                             "(the split decode for boxes is decode_jpeg_batch_split_crop / launch_jpeg_split_crop)")
        bx = _check_boxes(boxes, n, plan.grid)
        y_off, c_off, ny, ncc = packed_offsets(bx)
        if out is None:
            out = alloc_jpeg_packed(n, plan.grid, device)
        dev = upload_jpeg_plan(plan, out[0].device)
        out = (out[0], out[1], out[2][:n], out[3][:n])
        out[2].copy_(dev[4], non_blocking=True)
        out[3].copy_(dev[5], non_blocking=True)
        d = out[0].device
        packed = (y_off.to(d, non_blocking=True), c_off.to(d, non_blocking=True), ny, ncc)
        launch_jpeg_decode(plan, dev, out, boxes=bx.to(d, non_blocking=True), packed_out=packed)
        for t in dev[:4]:
            t.record_stream(torch.cuda.current_stream(d))
        return out[0][:ny], out[1][:ncc], out[2], out[3], packed[0], packed[1]
    if out is None:
        out = alloc_jpeg_out(n, plan.grid, device)
    out = tuple(t[:n] for t in out)
    dev = upload_jpeg_plan(plan, out[0].device)
    out[2].copy_(dev[4], non_blocking=True)
    out[3].copy_(dev[5], non_blocking=True)
    path = launch_jpeg_decode(plan, dev, out, split=True, seg_bits=seg_bits, rounds=rounds) if split else launch_jpeg_decode(plan, dev, out)
    for t in dev[:4]:                        # the launch reads them on this stream: keep the allocator from handing them out early
        t.record_stream(torch.cuda.current_stream(out[0].device))
    return out + (path,) if return_path else out


# ---- the split decode for a crop box per file (rgbnm_jpeg_decode_batch_split_crop) ------------------------------------------------
def jpeg_split_crop_scratch(plan, seg_bits=None, device="cuda"):
    """uint8 device tensor for launch_jpeg_split_crop(scratch=...) on this plan (or any with no more stream bytes and runs)."""
    from . import lib as L
    nbytes = L.lib().rgbnm_jpeg_split_crop_scratch_bytes(plan.stream_bytes, plan.nruns,
                                                         JPEG_SPLIT_SEG_BITS if seg_bits is None else int(seg_bits))
    if nbytes == 0:
        raise L.RgbnmError("seg_bits must be a multiple of 32 in 128..65536")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def launch_jpeg_split_crop(plan, dev, out, boxes, packed_out, path=None, scratch=None, seg_bits=None, rounds=None, walked=None,
                           seg_live=None):
    """The split decode for a crop box per file, the launches alone (no copy, no sync: capturable): launch_jpeg_decode(split=True)'s
    scout, sync and verify passes over the whole runs, then only the segments that hold a block of a file's box are walked, in dense
    waves, and only the boxes are stored, packed as launch_jpeg_decode(boxes=...) packs them.  For files without restart markers.
    dev: upload_jpeg_plan's tensors; out: (Ypacked, Cpacked, quant, status) device tensors (alloc_jpeg_packed), quant and status
    already holding the plan's; boxes: int32 (n, 4) DEVICE tensor; packed_out = (y_off, c_off, y_elems, c_elems) with int64 [n] device
    offsets; path int32 [n], scratch (jpeg_split_crop_scratch): from the caching allocator when None; seg_bits, rounds: the split
    decode's defaults; walked, seg_live: int32 [plan.nruns] device tensors or None -- the MCUs the one-lane walk took of each run, the
    segments the write pass walked of each split run.  The device checks every box and offset again (RGBNM_JPEG_EBOX).  Returns path."""
    from . import lib as L
    Y, CbCr, _, status = out
    hb, wb = plan.grid
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    n = plan.n
    if not torch.is_tensor(boxes) or packed_out is None:
        raise ValueError("boxes must be a device tensor and packed_out=(y_off, c_off, y_elems, c_elems) given: this is the capturable "
                         "launch (decode_jpeg_batch_split_crop uploads them)")
    y_off, c_off, ny, ncc = packed_out
    L.require_cuda(Y, CbCr, status, *dev[:4])
    L.require_cuda(boxes, y_off, c_off)
    seg_bits = JPEG_SPLIT_SEG_BITS if seg_bits is None else int(seg_bits)
    rounds = JPEG_SPLIT_ROUNDS if rounds is None else int(rounds)
    with torch.cuda.device(Y.device):
        if boxes.dtype != torch.int32 or tuple(boxes.shape) != (n, 4) or not boxes.is_contiguous():
            raise L.RgbnmError("boxes must be int32 (n, 4)")
        if any(t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous() for t in (y_off, c_off)):
            raise L.RgbnmError("y_off and c_off must be int64 [n]")
        if Y.dim() != 1 or CbCr.dim() != 1 or Y.dtype != torch.int16 or CbCr.dtype != torch.int16 or not Y.is_contiguous() \
                or not CbCr.is_contiguous() or int(ny) > Y.numel() or int(ncc) > CbCr.numel() or status.numel() != n \
                or status.dtype != torch.int32:
            raise L.RgbnmError("out tensors do not match the boxes (alloc_jpeg_packed)")
        for name, t in (("walked", walked), ("seg_live", seg_live)):
            if t is not None:
                L.require_cuda(t)
                if t.dtype != torch.int32 or t.numel() < plan.nruns or not t.is_contiguous():
                    raise L.RgbnmError(f"{name} must be int32 [plan.nruns]")
        if scratch is None:
            scratch = jpeg_split_crop_scratch(plan, seg_bits, Y.device)
        if path is None:
            path = torch.empty(n, dtype=torch.int32, device=Y.device)
        L.require_cuda(path, scratch)
        if path.dtype != torch.int32 or path.numel() != n or not path.is_contiguous() or scratch.dtype != torch.uint8 \
                or not scratch.is_contiguous():
            raise L.RgbnmError("path must be int32 [n], scratch uint8 (jpeg_split_crop_scratch)")
        dp = L.JpegDevicePlan(stream=dev[0].data_ptr(), stream_bytes=plan.stream_bytes, runs=dev[1].data_ptr(), images=dev[2].data_ptr(),
                              tables=dev[3].data_ptr(), nruns=plan.nruns, ntables=plan.ntables)
        L.check(L.lib().rgbnm_jpeg_decode_batch_split_crop(
            C.byref(dp), n, hb, wb, hbc, wbc, boxes.data_ptr(), y_off.data_ptr(), c_off.data_ptr(), Y.data_ptr(), int(ny), CbCr.data_ptr(),
            int(ncc), status.data_ptr(), path.data_ptr(), walked.data_ptr() if walked is not None else None,
            seg_live.data_ptr() if seg_live is not None else None, scratch.data_ptr(), scratch.numel(), seg_bits, rounds, L.stream()),
            "jpeg_decode_batch_split_crop")
    return path


def decode_jpeg_batch_split_crop(plan, device="cuda", boxes=None, out=None, seg_bits=None, rounds=None, return_path=False):
    """decode_jpeg_batch(boxes=...) through the split decode (launch_jpeg_split_crop), for files without restart markers: (Ypacked,
    Cpacked, quant, status, y_off, c_off), and the int32 path per file as a seventh with return_path=True.  The same packed bits.  For
    a file with path 1 the status is the whole decode's; for the others decode_jpeg_batch(boxes=...)'s caveat stands."""
    if boxes is None:
        raise ValueError("boxes are required (decode_jpeg_batch(split=True) decodes whole grids)")
    n = plan.n
    bx = _check_boxes(boxes, n, plan.grid)
    y_off, c_off, ny, ncc = packed_offsets(bx)
    if out is None:
        out = alloc_jpeg_packed(n, plan.grid, device)
    dev = upload_jpeg_plan(plan, out[0].device)
    out = (out[0], out[1], out[2][:n], out[3][:n])
    out[2].copy_(dev[4], non_blocking=True)
    out[3].copy_(dev[5], non_blocking=True)
    d = out[0].device
    packed = (y_off.to(d, non_blocking=True), c_off.to(d, non_blocking=True), ny, ncc)
    path = launch_jpeg_split_crop(plan, dev, out, bx.to(d, non_blocking=True), packed, seg_bits=seg_bits, rounds=rounds)
    for t in dev[:4]:
        t.record_stream(torch.cuda.current_stream(d))
    res = (out[0][:ny], out[1][:ncc], out[2], out[3], packed[0], packed[1])
    return res + (path,) if return_path else res


def jpeg_status_text(code):
    from . import lib as L
    return L.JPEG_STATUS.get(int(code), f"status {int(code)}")


def _raise_device_status(plan, status):
    """Raise, naming the first file whose device status is not 0 (synchronises to read it)."""
    st = status.cpu()
    if int((st != 0).sum()):
        i = int((st != 0).nonzero()[0])
        raise libjpeg_exception(f"{plan.names[i]}: device decode refused the file: {jpeg_status_text(st[i])}"
                                f"{' (' + plan.messages[i] + ')' if plan.messages[i] else ''} ({int((st != 0).sum())} of {plan.n} files failed)")


def read_coefficients_batch_device(paths_or_bytes, grid=(64, 64), device="cuda", split=False):
    """read_coefficients_batch with the entropy decode on the device: (Y, CbCr, quant) int16 DEVICE tensors.  Raises, naming the file,
    when one cannot be decoded there (synchronises to read the device status).  split: the split decode (decode_jpeg_batch)."""
    plan = prepare_jpeg_batch(paths_or_bytes, grid)
    Y, CbCr, quant, status = decode_jpeg_batch(plan, device, split=split)
    _raise_device_status(plan, status)
    return Y, CbCr, quant


def read_coefficients_batch_crop_device(paths_or_bytes, boxes, grid=(64, 64), device="cuda", split=False):
    """read_coefficients_batch_crop with the entropy decode on the device: (Ypacked, Cpacked, quant, y_off, c_off), all DEVICE
    tensors.  A bad box raises the host crop reader's ValueError; a file the device cannot decode raises, naming it (synchronises to
    read the device status).  split: the split decode for boxes (decode_jpeg_batch_split_crop), for files without restart markers."""
    bx = _check_boxes(boxes, len(paths_or_bytes), grid)
    plan = prepare_jpeg_batch(paths_or_bytes, grid)
    decode = decode_jpeg_batch_split_crop if split else decode_jpeg_batch
    Yp, Cp, quant, status, y_off, c_off = decode(plan, device, boxes=bx)
    _raise_device_status(plan, status)
    return Yp, Cp, quant, y_off, c_off


# ---- pixels <-> coefficients on the device (csrc/pixel_dct.hip) --------------------------------------------------------------
# ITU-T T.81 Annex K, natural order
_LUMA_TABLE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_CHROMA_TABLE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def quality_tables(quality, channels=3, baseline=True):
    """int16 (channels,8,8) CPU tensor: the standard tables at `quality` (1..100) as libjpeg's jpeg_set_quality scales them; the
    chroma table twice for three channels."""
    from . import lib as L
    q = int(quality)
    if not 1 <= q <= 100:
        raise L.RgbnmError(f"quality must be in 1..100, got {quality}")
    if channels not in (1, 3):
        raise L.RgbnmError(f"1 or 3 channels, got {channels}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    top = 255 if baseline else 32767
    base = torch.tensor([_LUMA_TABLE, _CHROMA_TABLE, _CHROMA_TABLE][:channels], dtype=torch.int64)
    return ((base * s + 50) // 100).clamp(1, top).to(torch.int16).reshape(channels, 8, 8)


def _host_table(quant, channels):
    """The table as a contiguous int16 CPU tensor (a device tensor is copied back: that synchronises and cannot be captured)."""
    from . import lib as L
    if not torch.is_tensor(quant) or quant.dtype != torch.int16 or tuple(quant.shape[-2:]) != (8, 8) or quant.numel() < 64 * channels:
        raise L.RgbnmError(f"quant must be an int16 tensor ({channels},8,8)")
    return quant.detach().cpu().reshape(-1, 8, 8)[:channels].contiguous()


def quantize_at_quality(pixels, quality, baseline=True):
    """(dim, quant, Y, CbCr|None) of uint8 pixels (C,H,W) or a batch (B,C,H,W) on a HIP device -- reference:
    dct_manip.quantize_at_quality (dct_manip.cpp:315-375), i.e. libjpeg at 4:2:0 without the entropy coder.
    dim int32 [[H,W],[H/2,W/2],[H/2,W/2]] ([[H,W]] for one channel) and quant int16 (C,8,8) are CPU tensors; Y int16
    ([B,]1,H/8,W/8,8,8) and CbCr int16 ([B,]2,H/16,W/16,8,8) are on the device.  C = 3 needs H and W divisible by 16, C = 1 by 8.
    Luma equals libjpeg bit for bit, chroma is within 1 of it."""
    from . import lib as L
    if not torch.is_tensor(pixels):
        raise TypeError(f"pixels must be a uint8 tensor on the device, got {type(pixels).__name__}")
    if pixels.dtype != torch.uint8:
        raise L.RgbnmError(f"pixels must be uint8, got {pixels.dtype}")
    if pixels.dim() not in (3, 4):
        raise L.RgbnmError(f"pixels must be (C,H,W) or (B,C,H,W), got {tuple(pixels.shape)}")
    batched = pixels.dim() == 4
    B = pixels.shape[0] if batched else 1
    Cn, H, W = (int(v) for v in pixels.shape[-3:])
    if Cn not in (1, 3):
        raise L.RgbnmError(f"1 (gray) or 3 (RGB) channels, got {Cn}")
    mod = 16 if Cn == 3 else 8
    if B < 1 or H < mod or W < mod or H % mod or W % mod:
        raise L.RgbnmError(f"height and width must be multiples of {mod} for {Cn} channel(s) (no edge replication), got {H} x {W}")
    quant = quality_tables(quality, Cn, baseline)
    L.require_cuda(pixels)
    lead = (B,) if batched else ()
    Y = torch.empty(lead + (1, H // 8, W // 8, 8, 8), dtype=torch.int16, device=pixels.device)
    CbCr = torch.empty(lead + (2, H // 16, W // 16, 8, 8), dtype=torch.int16, device=pixels.device) if Cn == 3 else None
    with torch.cuda.device(pixels.device):
        L.check(L.lib().rgbnm_pixels_to_dct(pixels.data_ptr(), B, Cn, H, W, quant.data_ptr(), Y.data_ptr(), L.ptr(CbCr), L.stream()),
                "pixels_to_dct")
    dim = torch.tensor([[H, W], [H // 2, W // 2], [H // 2, W // 2]][:Cn], dtype=torch.int32)
    return dim, quant, Y, CbCr


def decode_coeff(dim, quant, Y, CbCr=None, quality=-1):
    """uint8 pixels (C,H,W) or (B,C,H,W) on the device from int16 coefficients Y ([B,]1,Hb,Wb,8,8) and CbCr ([B,]2,Hb/2,Wb/2,8,8)
    or None (one channel) -- reference: dct_manip.decode_coeff (dct_manip.cpp:485-576).  quant int16 (C,8,8), best on the CPU (a
    device table is copied back first); quality > 0 replaces it by the standard tables, as in the reference.  dim is checked
    against the grids when given (None: inferred).  Within 3 of libjpeg wherever the exact plane samples lie in [-128, 383];
    outside that range libjpeg wraps around and this call saturates."""
    from . import lib as L
    if Y.dtype != torch.int16 or (CbCr is not None and CbCr.dtype != torch.int16):
        raise L.RgbnmError("coefficients must be int16")
    if Y.dim() not in (5, 6) or tuple(Y.shape[-2:]) != (8, 8) or Y.shape[-5] != 1:
        raise L.RgbnmError(f"Y must be ([B,]1,Hb,Wb,8,8), got {tuple(Y.shape)}")
    batched = Y.dim() == 6
    B = Y.shape[0] if batched else 1
    Hb, Wb = int(Y.shape[-4]), int(Y.shape[-3])
    Cn = 1 if CbCr is None else 3
    if CbCr is not None:
        want = ((B,) if batched else ()) + (2, Hb // 2, Wb // 2, 8, 8)
        if Hb % 2 or Wb % 2 or tuple(CbCr.shape) != want:
            raise L.RgbnmError(f"CbCr must be {want} for Y {tuple(Y.shape)} (even luma grid, 4:2:0), got {tuple(CbCr.shape)}")
    if B < 1 or Hb < 1 or Wb < 1:
        raise L.RgbnmError(f"empty coefficient grid {tuple(Y.shape)}")
    H, W = 8 * Hb, 8 * Wb
    if dim is not None and [int(v) for v in torch.as_tensor(dim).reshape(-1)[:2]] != [H, W]:
        raise L.RgbnmError(f"dim says {[int(v) for v in torch.as_tensor(dim).reshape(-1)[:2]]}, the luma grid is {H} x {W} "
                           "(sizes that need edge replication are not supported)")
    table = quality_tables(quality, Cn) if quality > 0 else _host_table(quant, Cn)
    L.require_cuda(Y, CbCr)
    out = torch.empty(((B,) if batched else ()) + (Cn, H, W), dtype=torch.uint8, device=Y.device)
    with torch.cuda.device(Y.device):
        L.check(L.lib().rgbnm_dct_to_pixels(Y.data_ptr(), L.ptr(CbCr), B, H, W, table.data_ptr(), out.data_ptr(), L.stream()),
                "dct_to_pixels")
    return out


# ---- coefficients -> JPEG files on the device (csrc/jpeg_emit.h, jpeg_encode.hip) --------------------------------------------
def _restart_interval(restart, mcus_x):
    if restart == "row":
        return int(mcus_x)
    if isinstance(restart, str) or not 0 <= int(restart) <= 65535:
        raise ValueError(f'restart must be 0..65535 MCUs or "row", got {restart!r}')
    return int(restart)


def _encode_grids(Y, CbCr):
    from . import lib as L
    if not torch.is_tensor(Y) or Y.dtype != torch.int16 or Y.dim() != 6 or tuple(Y.shape[1:2] + Y.shape[4:]) != (1, 8, 8):
        raise L.RgbnmError(f"Y must be int16 (n,1,Hb,Wb,8,8), got {tuple(Y.shape) if torch.is_tensor(Y) else type(Y).__name__}")
    n, hb, wb = int(Y.shape[0]), int(Y.shape[2]), int(Y.shape[3])
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    if CbCr is not None and (CbCr.dtype != torch.int16 or tuple(CbCr.shape) != (n, 2, hbc, wbc, 8, 8)):
        raise L.RgbnmError(f"CbCr must be int16 {(n, 2, hbc, wbc, 8, 8)} for Y {tuple(Y.shape)} (4:2:0), got {tuple(CbCr.shape)}")
    if n < 1 or hb < 1 or wb < 1:
        raise L.RgbnmError(f"empty coefficient grid {tuple(Y.shape)}")
    return n, hb, wb, hbc, wbc


def _encode_quant(quant, n, ch, dev):
    """int16 (n,ch,64) on dev from (C,8,8) / (C,64) for all images or (n,C,8,8) / (n,C,64), C >= ch (the decode returns three)."""
    from . import lib as L
    q = torch.as_tensor(quant)
    if q.dtype == torch.int16 and q.dim() >= 2 and tuple(q.shape[-2:]) == (8, 8):
        q = q.reshape(q.shape[:-2] + (64,))
    if q.dtype != torch.int16 or q.dim() not in (2, 3) or q.shape[-1] != 64 or q.shape[-2] < ch or (q.dim() == 3 and q.shape[0] != n):
        raise L.RgbnmError(f"quant must be int16 ({ch},8,8) or ({n},{ch},8,8), got {q.dtype} {tuple(q.shape)}")
    if q.dim() == 2:
        q = q.unsqueeze(0).expand(n, q.shape[0], 64)
    return q[:, :ch].to(dev).contiguous()


def jpeg_encode_header_bytes(channels=3, restart=0):
    """Size of the header encode_jpeg_batch writes (SOI through the SOS header)."""
    return (623 if channels == 3 else 328) + (6 if restart else 0)


def _default_stride(ch, ri, hb, wb):
    """The header plus one byte per coefficient of the kept grids."""
    return jpeg_encode_header_bytes(ch, ri) + 64 * (hb * wb + (2 * ((hb + 1) // 2) * ((wb + 1) // 2) if ch == 3 else 0))


def jpeg_encode_bound(grid, channels=3, restart=0):
    """Worst-case size of a file of luma grid (Hb, Wb): a stride that never gives 'plan buffers too small' (rgbnm_jpeg_encode_bound)."""
    from . import lib as L
    hb, wb = (int(v) for v in grid)
    mx = (wb + 1) // 2 if channels == 3 else wb
    b = L.lib().rgbnm_jpeg_encode_bound(hb, wb, (hb + 1) // 2, (wb + 1) // 2, int(channels), _restart_interval(restart, mx))
    if b == 0:
        raise L.RgbnmError(f"grid {grid} with {channels} channel(s), restart {restart}: not a layout the encoder writes")
    return int(b)


def jpeg_encode_header(height, width, quant, restart=0):
    """The header bytes of one file, SOI through the SOS header, as the device writes them (host only: rgbnm_jpeg_encode_header).
    quant int16 (C,8,8), C = 1 or 3."""
    from . import lib as L
    q = torch.as_tensor(quant).detach().cpu().to(torch.int16).reshape(-1, 64).contiguous()
    if q.shape[0] not in (1, 3):
        raise L.RgbnmError("quant must be int16 (1,8,8) or (3,8,8)")
    buf = (C.c_uint8 * 640)()
    mx = -(-int(width) // (16 if q.shape[0] == 3 else 8))
    rc = L.lib().rgbnm_jpeg_encode_header(int(q.shape[0]), int(height), int(width), q.data_ptr(), _restart_interval(restart, mx), buf, 640)
    if rc < 0:
        L.check(rc, "jpeg_encode_header")
    return bytes(buf[:rc])


def jpeg_encode_scratch(n, grid, channels=3, restart=0, stride=None, device="cuda"):
    """uint8 device tensor for encode_jpeg_batch(scratch=...) with these arguments (restart as an interval in MCUs or "row")."""
    from . import lib as L
    hb, wb = (int(v) for v in grid)
    hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
    ri = _restart_interval(restart, wbc if channels == 3 else wb)
    if stride is None:
        stride = _default_stride(channels, ri, hb, wb)
    nbytes = L.lib().rgbnm_jpeg_encode_scratch_bytes(int(n), hb, wb, hbc, wbc, int(channels), ri, int(stride))
    if nbytes == 0:
        raise L.RgbnmError(f"n {n}, grid {grid}, {channels} channel(s), restart {restart}, stride {stride}: not a call the encoder takes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def encode_jpeg_batch(Y, CbCr, quant, dims=None, restart=0, stride=None, out=None, scratch=None):
    """Whole baseline JPEG files from coefficient tensors ON THE DEVICE (rgbnm_jpeg_encode_batch; there is no CPU fallback): four
    launches, no copy and no host synchronisation when every argument already is a device tensor, so the call can be captured.
    Y int16 (n,1,Hb,Wb,8,8), CbCr int16 (n,2,ceil(Hb/2),ceil(Wb/2),8,8) or None (one component); quant int16 (n,C,8,8) as
    decode_jpeg_batch returns it, or (C,8,8) for all images (table 1 serves both chroma planes); dims int32 (n,2) [height, width]
    per image, or None: 8 Hb x 8 Wb.  restart: the restart interval in MCUs, 0 for none, "row" for one interval per MCU row (the
    layout the plain device decode is fast on).  stride: bytes per file slot; None: the header plus one byte per coefficient.
    out: (buf uint8 (n,stride), nbytes int32 (n), status int32 (n)) to write into.  Returns (buf, nbytes, status) on the device:
    status 0, or a negative code (jpeg_status_text) with nbytes 0 and the slot untouched -- "DCT coefficient out of range" for an AC
    coefficient beyond +-1023 or a DC step beyond +-2047, "plan buffers too small" when the file is longer than stride
    (jpeg_encode_bound never is), "grid differs" when dims does not give the tensors' grids.  The files are what libjpeg's
    jpeg_write_coefficients writes (the reference's write_coefficients), byte for byte."""
    from . import lib as L
    n, hb, wb, hbc, wbc = _encode_grids(Y, CbCr)
    ch = 1 if CbCr is None else 3
    L.require_cuda(Y, CbCr)
    dev = Y.device
    ri = _restart_interval(restart, wbc if ch == 3 else wb)
    quant = _encode_quant(quant, n, ch, dev)
    if dims is None:
        dims = torch.tensor([[8 * hb, 8 * wb]] * n, dtype=torch.int32)
    dims = torch.as_tensor(dims)
    if dims.dtype != torch.int32 or dims.numel() != 2 * n:
        raise L.RgbnmError(f"dims must be int32 (n,2) [height, width], got {dims.dtype} {tuple(dims.shape)}")
    dims = dims.reshape(n, 2).to(dev).contiguous()
    if stride is None:
        stride = _default_stride(ch, ri, hb, wb)
    stride = int(stride)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((n, stride), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev))
        buf, nbytes, status = out
        L.require_cuda(buf, nbytes, status)
        if buf.dtype != torch.uint8 or tuple(buf.shape) != (n, stride) or nbytes.dtype != torch.int32 or nbytes.numel() != n \
                or status.dtype != torch.int32 or status.numel() != n:
            raise L.RgbnmError(f"out must be (uint8 ({n},{stride}), int32 ({n}), int32 ({n}))")
        if scratch is None:
            scratch = jpeg_encode_scratch(n, (hb, wb), ch, ri, stride, dev)
        L.require_cuda(scratch)
        if scratch.dtype != torch.uint8:
            raise L.RgbnmError("scratch must be uint8 (jpeg_encode_scratch)")
        L.check(L.lib().rgbnm_jpeg_encode_batch(Y.data_ptr(), L.ptr(CbCr), quant.data_ptr(), dims.data_ptr(), n, hb, wb, hbc, wbc, ri,
                                                buf.data_ptr(), stride, nbytes.data_ptr(), status.data_ptr(), scratch.data_ptr(),
                                                scratch.numel(), L.stream()), "jpeg_encode_batch")
    return buf, nbytes, status


def encode_jpeg_files(Y, CbCr, quant, dims=None, restart=0):
    """encode_jpeg_batch, then the files as a list of bytes on the host (synchronises).  An image whose file did not fit the default
    stride is encoded again with the worst-case stride; any other failure raises libjpeg_exception, with the reference's wording
    ("DCT coefficient out of range") for a value baseline Huffman coding cannot express."""
    from . import lib as L
    n, hb, wb, _, _ = _encode_grids(Y, CbCr)
    buf, nbytes, status = encode_jpeg_batch(Y, CbCr, quant, dims, restart)
    st, nb = status.cpu(), nbytes.cpu()
    host = buf.cpu()
    files = [bytes(host[i, :int(nb[i])].numpy().tobytes()) for i in range(n)]
    again = [i for i in range(n) if int(st[i]) == -15]
    if again:
        idx = torch.tensor(again, device=Y.device)
        q = _encode_quant(quant, n, 1 if CbCr is None else 3, Y.device).index_select(0, idx)
        d = None if dims is None else torch.as_tensor(dims).reshape(n, 2).to(Y.device).index_select(0, idx)
        b2, n2, s2 = encode_jpeg_batch(Y.index_select(0, idx).contiguous(), None if CbCr is None else CbCr.index_select(0, idx).contiguous(),
                                       q, d, restart, stride=jpeg_encode_bound((hb, wb), 1 if CbCr is None else 3, restart))
        b2, n2, s2 = b2.cpu(), n2.cpu(), s2.cpu()
        for k, i in enumerate(again):
            st[i] = s2[k]
            files[i] = bytes(b2[k, :int(n2[k])].numpy().tobytes())
    for i in range(n):
        if int(st[i]) != 0:
            text = jpeg_status_text(st[i])
            raise libjpeg_exception(text if int(st[i]) == -25 else f"image {i}: device encode refused the image: {text}")
    return files


def write_coefficients_batch(paths, dims, quant, Y, CbCr=None, restart=0):
    """One file per image of a batch: Y int16 (n,1,Hb,Wb,8,8), CbCr int16 (n,2,Hbc,Wbc,8,8) or None, quant int16 (n,C,8,8) or (C,8,8),
    dims int32 (n,2) [height, width] or None; tensors on the CPU are copied to the device, where the encode always runs.  restart as
    in encode_jpeg_batch: restart="row" writes files the plain device decode reads at full speed (a lossless transcode when the
    coefficients came from decode_jpeg_batch)."""
    from . import lib as L
    paths = list(paths)
    if not torch.is_tensor(Y) or Y.dim() != 6 or len(paths) != Y.shape[0]:
        raise L.RgbnmError("one path per image of Y (n,1,Hb,Wb,8,8)")
    if not Y.is_cuda:
        if not torch.cuda.is_available():
            raise L.RgbnmError("write_coefficients encodes on the device (HIP); there is no CPU fallback")
        Y = Y.to("cuda")
    if CbCr is not None:
        CbCr = CbCr.to(Y.device)
    files = encode_jpeg_files(Y.contiguous(), None if CbCr is None else CbCr.contiguous(), quant, dims, restart)
    for p, data in zip(paths, files):
        try:
            fh = open(p, "wb")
        except OSError:
            raise RuntimeError(f"Unable to open file for reading: {p}") from None      # the reference's wording, dct_manip.cpp:271-275
        with fh:
            fh.write(data)


def write_coefficients(path, dimensions, quantization, Y, CbCr=None):
    """Reference: dct_manip.write_coefficients (dct_manip.cpp:265-313) with its argument layout -- dimensions int32 [[H,W],...] (row 0
    is used), quantization int16 (C,8,8) (table 1 serves both chroma planes), Y int16 (1,Hb,Wb,8,8), CbCr int16 (2,Hbc,Wbc,8,8) or
    None -- and its file, byte for byte: standard Huffman tables, 4:2:0, no restart markers.  The encode runs on the device (CPU
    tensors are copied there).  Raises libjpeg_exception("DCT coefficient out of range") like the reference."""
    from . import lib as L
    if not torch.is_tensor(Y) or Y.dim() != 5:
        raise L.RgbnmError("Y must be int16 (1,Hb,Wb,8,8)")
    dim = torch.as_tensor(dimensions).reshape(-1, 2)[:1].to(torch.int32)
    write_coefficients_batch([path], dim, torch.as_tensor(quantization).reshape(-1, 8, 8), Y.unsqueeze(0),
                             None if CbCr is None else CbCr.unsqueeze(0))
