"""The device JPEG encode (csrc/jpeg_encode.hip: measure, place, emit, stuff) -- every comparison is exact equality of bytes or int16
values: against the reference's files (tests/golden/g26_jpeg_write.npz), against the plain-Python writer from the SOS header on with
and without restart markers, through the host libjpeg reader and the device decode, and at the batch's edges into guarded outputs."""
import functools

import numpy as np
import pytest
import torch

import kernel_check as KC
from jpeg_encode_ref import CASES, case, scan_start, writer_file
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu

ERANGE, ECAPACITY, EGRID = -25, -15, -13
SIZES = [(8, 8), (16, 16), (24, 40), (17, 9), (96, 112), (144, 16)]       # height x width; the last: 9 MCU rows of one MCU


def grids(h, w):
    return (-(-h // 8), -(-w // 8)), (-(-h // 16), -(-w // 16))


def random_image(seed, h, w, gray=False, amp=40, keep=0.3, dc=200):
    """(quant (C,8,8), Y (1,Hb,Wb,8,8), C (2,Hbc,Wbc,8,8) | None) int16"""
    r = np.random.RandomState(seed)
    (hb, wb), (hc, wc) = grids(h, w)

    def plane(*lead):
        x = r.randint(-amp, amp + 1, lead + (8, 8)) * (r.rand(*lead, 8, 8) < keep)
        x[..., 0, 0] = r.randint(-dc, dc + 1, lead)
        return x.astype(np.int16)

    return r.randint(1, 256, (1 if gray else 3, 8, 8)).astype(np.int16), plane(1, hb, wb), None if gray else plane(2, hc, wc)


def to_device(images):
    """images [(quant, Y, C | None)] of one grid -> (Y, CbCr | None, quant) batch tensors on the device"""
    Y = torch.from_numpy(np.stack([im[1] for im in images])).cuda()
    Cc = None if images[0][2] is None else torch.from_numpy(np.stack([im[2] for im in images])).cuda()
    return Y, Cc, torch.from_numpy(np.stack([im[0] for im in images])).cuda()


def dims_of(n, h, w):
    return torch.tensor([[h, w]] * n, dtype=torch.int32, device="cuda")


def files_of(buf, nbytes):
    b, nb = buf.cpu().numpy(), nbytes.tolist()
    return [b[i, :nb[i]].tobytes() for i in range(len(nb))]


def from_sos(data, gray):
    return data[scan_start(data) - (10 if gray else 14):]


@functools.lru_cache(maxsize=None)
def oracle(seed, h, w, gray, restart):
    q, Y, Cc = random_image(seed, h, w, gray)
    return writer_file(h, w, q, Y, Cc, restart)


@pytest.mark.parametrize("name", CASES)
def test_write_coefficients_reproduces_the_reference_file(name, tmp_path, golden):
    h, w, quant, Y, Cc, data = case(golden("g26_jpeg_write.npz"), name)
    dim = torch.from_numpy(golden("g26_jpeg_write.npz")[f"{name}_dim"].copy())
    path = str(tmp_path / f"{name}.jpg")
    dm.write_coefficients(path, dim, torch.from_numpy(quant.copy()), torch.from_numpy(Y.copy()), None if Cc is None else torch.from_numpy(Cc.copy()))
    assert open(path, "rb").read() == data
    # device tensors, and the batched call with one restart interval per MCU row: the same coefficients come back
    dm.write_coefficients_batch([path], dim[:1], torch.from_numpy(quant.copy()), torch.from_numpy(Y.copy()).cuda()[None],
                                None if Cc is None else torch.from_numpy(Cc.copy()).cuda()[None], restart="row")
    _, q2, Y2, C2 = dm.read_coefficients(path)
    assert Y2.numpy().tobytes() == Y.tobytes() and (Cc is None or C2.numpy().tobytes() == Cc.tobytes())
    assert q2[:2].numpy().tobytes() == quant[:2].tobytes()


def test_out_of_range_raises_with_the_reference_wording(tmp_path, golden):
    h, w, quant, Y, Cc, _ = case(golden("g26_jpeg_write.npz"), "r24x40")
    Y = Y.copy()
    Y[0, 1, 2, 3, 4] = 1024
    with pytest.raises(dm.libjpeg_exception, match="^DCT coefficient out of range$"):
        dm.write_coefficients(str(tmp_path / "x.jpg"), torch.tensor([[h, w]], dtype=torch.int32), torch.from_numpy(quant.copy()),
                              torch.from_numpy(Y), torch.from_numpy(Cc.copy()))
    assert not (tmp_path / "x.jpg").exists()


@pytest.mark.parametrize("h,w,gray", [s + (False,) for s in SIZES] + [(24, 40, True), (17, 9, True), (144, 16, True)])
def test_against_the_python_writer_and_both_decoders(h, w, gray):
    """n = 2 per call.  From the SOS header on the files equal jpeg_writer's for restart 0, 1, 4, "row" and one above the MCU count;
    the host reader and the plain device decode give the inputs back.  RSTn goes round from RST7 to RST0 wherever a file has more
    than nine runs: 96 x 112 at intervals 1 and 4, the gray 144 x 16 (18 block rows) at "row"; the 4:2:0 144 x 16 at "row" has nine
    runs and ends on RST7."""
    (hb, wb), (hc, wc) = grids(h, w)
    mx, nmcu = (wb, hb * wb) if gray else (wc, hc * wc)
    seeds = (h * 1000 + w, h * 1000 + w + 1)
    images = [random_image(s, h, w, gray) for s in seeds]
    Y, Cc, quant = to_device(images)
    for restart in (0, 1, 4, "row", nmcu + 1):
        ri = mx if restart == "row" else restart
        buf, nbytes, status = dm.encode_jpeg_batch(Y, Cc, quant, dims_of(2, h, w), restart=restart)
        assert status.tolist() == [0, 0], (restart, status.tolist())
        files = files_of(buf, nbytes)
        for i, data in enumerate(files):
            ref = oracle(seeds[i], h, w, gray, ri)
            assert from_sos(data, gray) == from_sos(ref, gray), (restart, i)
            assert data[:scan_start(data)] == dm.jpeg_encode_header(h, w, images[i][0], ri)
            _, q, Yh, Ch = dm.read_coefficients_bytes(data)
            assert Yh.numpy().tobytes() == images[i][1].tobytes() and (gray or Ch.numpy().tobytes() == images[i][2].tobytes())
            assert q[:2].numpy().tobytes() == images[i][0][:2].tobytes()
        plan = dm.prepare_jpeg_batch(files, grid=(hb, wb))
        assert plan.nbad == 0 and plan.nruns == 2 * -(-nmcu // min(ri or nmcu, nmcu)), plan.messages
        Yd, Cd, Qd, st = dm.decode_jpeg_batch(plan, "cuda")
        assert st.tolist() == [0, 0] and torch.equal(Yd, Y) and (gray or torch.equal(Cd, Cc))
        assert torch.equal(Qd[:, :1 if gray else 2], quant[:, :1 if gray else 2])


def test_decode_encode_decode_is_lossless():
    """Device decode (files without restart markers) -> encode with one restart interval per MCU row -> device decode: the first
    decode's tensors and tables; the files in between have one run per MCU row."""
    import jpeg_cases as JC
    p = JC.pillow_files()
    files = [p["q75"], p["q30"], p["rst_rows1"]]
    plan = dm.prepare_jpeg_batch(files, grid=(9, 13))
    assert plan.nbad == 0
    Y, Cc, Q, st = dm.decode_jpeg_batch(plan, "cuda")
    assert st.tolist() == [0, 0, 0]
    buf, nbytes, status = dm.encode_jpeg_batch(Y, Cc, Q, restart="row")
    assert status.tolist() == [0, 0, 0]
    again = dm.prepare_jpeg_batch(files_of(buf, nbytes), grid=(9, 13))
    assert again.nbad == 0 and again.nruns == 3 * 5                  # 9 block rows: 5 MCU rows
    Y2, C2, Q2, st2 = dm.decode_jpeg_batch(again, "cuda")
    assert st2.tolist() == [0, 0, 0] and torch.equal(Y2, Y) and torch.equal(C2, Cc) and torch.equal(Q2[:, :2], Q[:, :2])
    assert torch.equal(Q2[:, 2], Q[:, 1])                             # table 1 serves both chroma planes in the written file


# ---- batch edges ------------------------------------------------------------------------------------------------------------------
H5, W5 = 40, 56                                                       # 5 x 7 blocks: partial MCUs on both edges


@functools.lru_cache(maxsize=None)
def mixed():
    """Five images: nearly empty, dense, one with an AC coefficient of 1024, two ordinary ones; the oracle's files (None: ERANGE) and
    the sizes the encoder's files must have: the oracle's plus the 18 bytes of APP0, which jpeg_writer does not write."""
    images = [random_image(70 + k, H5, W5) for k in range(5)]
    images[0] = (images[0][0], np.zeros_like(images[0][1]), np.zeros_like(images[0][2]))
    images[0][1][0, 4, 6, 0, 0] = -3
    images[1] = random_image(71, H5, W5, amp=300, keep=0.6, dc=1000)
    images[2][2][1, 2, 3, 7, 7] = 1024
    want = [None if k == 2 else writer_file(H5, W5, *images[k], 0) for k in range(5)]
    return images, want, [0 if f is None else len(f) + 18 for f in want]


class Slots:
    """out / nbytes / status for n files inside canary-filled buffers (stride even)."""

    def __init__(self, n, stride):
        assert stride % 2 == 0
        self.g = [KC.guarded(n, stride // 2, torch.int16), KC.guarded(n, None, torch.int32), KC.guarded(n, None, torch.int32)]
        self.t = (self.g[0].t.view(torch.uint8), self.g[1].t, self.g[2].t)
        self.canary = bytes([self.g[0].canary & 255, self.g[0].canary >> 8])

    def check(self, where):
        torch.cuda.synchronize()
        self.g[0].check(f"{where} out", written=False)
        self.g[1].check(f"{where} nbytes")
        self.g[2].check(f"{where} status")

    def slot(self, i):
        return self.t[0][i].cpu().numpy().tobytes()


def encode_mixed(stride, where, **kw):
    images = mixed()[0]
    Y, Cc, quant = to_device(images)
    out = Slots(5, stride)
    buf, nbytes, status = dm.encode_jpeg_batch(Y, Cc, quant, dims_of(5, H5, W5), stride=stride, out=out.t, **kw)
    out.check(where)
    return out, nbytes.tolist(), status.tolist()


def check_mixed(out, nbytes, status, failed, where):
    """`failed`: {image: status}.  Every other image holds the oracle's file; what lies behind a file, and a failed image's whole
    slot, still holds the canary."""
    images, want, size = mixed()
    stride = out.t[0].shape[1]
    for i in range(5):
        slot = out.slot(i)
        if i in failed:
            assert (status[i], nbytes[i]) == (failed[i], 0), (where, i, status, nbytes)
            assert slot == out.canary * (stride // 2), (where, i, "a failed image's slot was written")
            continue
        assert (status[i], nbytes[i]) == (0, size[i]), (where, i, status, nbytes)
        assert from_sos(slot[:nbytes[i]], False) == from_sos(want[i], False), (where, i)
        assert slot[:623] == dm.jpeg_encode_header(H5, W5, images[i][0]), (where, i)
        tail = slot[nbytes[i]:]
        assert tail == (out.canary * (stride // 2))[nbytes[i]:], (where, i, "bytes behind the file were written")


def test_mixed_batch_status_sizes_and_untouched_slots():
    size = mixed()[2]
    sizes = [v for v in size if v]
    assert min(sizes) < 700 and max(sizes) > 4 * min(sizes)          # nearly empty: the header and a few bytes; dense: kilobytes
    stride = max(sizes) + 6 + max(sizes) % 2
    out, nbytes, status = encode_mixed(stride, "mixed")
    check_mixed(out, nbytes, status, {2: ERANGE}, "mixed")
    first = [out.slot(i) for i in range(5)]
    # the same call again, and with one and two workgroups per launch: the same bytes
    for wgs in (0, 1, 2):
        L.set_option("jpeg_encode_wgs", wgs)
        try:
            out2, nbytes2, status2 = encode_mixed(stride, f"{wgs} workgroups")
        finally:
            L.set_option("jpeg_encode_wgs", 0)
        assert (nbytes2, status2) == (nbytes, status) and [out2.slot(i) for i in range(5)] == first, wgs
    # a stride one byte short of the longest file (kept even for the guard words: the file is the only one of its size or one less)
    k = max(range(5), key=lambda i: size[i])
    short = size[k] - 1 - (size[k] - 1) % 2
    assert sorted(sizes)[-2] <= short < size[k]
    out3, nbytes3, status3 = encode_mixed(short, "short stride")
    check_mixed(out3, nbytes3, status3, {2: ERANGE, k: ECAPACITY}, "short stride")
    out4, nbytes4, status4 = encode_mixed(size[k] + size[k] % 2, "exact stride")
    check_mixed(out4, nbytes4, status4, {2: ERANGE}, "exact stride")


def test_capacity_is_exact_to_the_byte_and_dims_are_checked():
    images, want, size = mixed()
    Y, Cc, quant = to_device([images[3]])
    n = size[3]
    for stride, st in ((n - 1, ECAPACITY), (n, 0), (n + 1, 0)):
        buf, nbytes, status = dm.encode_jpeg_batch(Y, Cc, quant, dims_of(1, H5, W5), stride=stride)
        assert status.tolist() == [st] and nbytes.tolist() == [n if st == 0 else 0], stride
        assert st != 0 or from_sos(files_of(buf, nbytes)[0], False) == from_sos(want[3], False)
    # write_coefficients_batch never shows ECAPACITY: the dense image does not fit the default stride and is encoded again
    dense = random_image(5, 16, 16, amp=1023, keep=1.0)
    Yd, Cd, qd = to_device([dense, random_image(6, 16, 16)])
    _, nb, st = dm.encode_jpeg_batch(Yd, Cd, qd)
    assert st.tolist() == [ECAPACITY, 0] and nb[0].item() == 0
    files = dm.encode_jpeg_files(Yd, Cd, qd)
    assert from_sos(files[0], False) == from_sos(writer_file(16, 16, *dense, 0), False) and len(files[0]) > 623 + 64 * 6
    assert len(files[0]) <= dm.jpeg_encode_bound((2, 2))
    # dims that do not give the tensors' grids
    dims = torch.tensor([[H5, W5], [H5 + 1, W5], [H5, W5 - 8], [33, 49]], dtype=torch.int32, device="cuda")
    Y4, C4, q4 = to_device([images[3]] * 4)
    _, nb, st = dm.encode_jpeg_batch(Y4, C4, q4, dims)
    assert st.tolist() == [0, EGRID, EGRID, 0] and nb.tolist()[1:3] == [0, 0] and nb[0].item() == n


def test_full_size_grid_the_prefix_loop_goes_round():
    """64 x 64 blocks at n = 2: 6144 + 2048 blocks per image, 32 trips of the placing loop; read back by the host reader."""
    images = [random_image(90 + k, 512, 512, keep=0.06) for k in range(2)]
    Y, Cc, quant = to_device(images)
    buf, nbytes, status = dm.encode_jpeg_batch(Y, Cc, quant, restart=0)
    assert status.tolist() == [0, 0]
    row, _, st = dm.encode_jpeg_batch(Y, Cc, quant, restart="row")
    assert st.tolist() == [0, 0]
    for i, data in enumerate(files_of(buf, nbytes)):
        _, _, Yh, Ch = dm.read_coefficients_bytes(data)
        assert Yh.numpy().tobytes() == images[i][1].tobytes() and Ch.numpy().tobytes() == images[i][2].tobytes()
        assert data.endswith(b"\xff\xd9")


def test_graph_capture_and_replay_with_other_coefficients():
    sets = [to_device([random_image(40 + 2 * s + k, 24, 40) for k in range(2)]) for s in range(2)]
    dims = dims_of(2, 24, 40)
    eager = [tuple(t.clone() for t in dm.encode_jpeg_batch(*s, dims, restart=2)) for s in sets]
    assert not torch.equal(eager[0][0], eager[1][0])
    Y, Cc, quant = (t.clone() for t in sets[0])
    stride = eager[0][0].shape[1]
    out = (torch.zeros((2, stride), dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
           torch.zeros(2, dtype=torch.int32, device="cuda"))
    scratch = dm.jpeg_encode_scratch(2, (3, 5), 3, 2, stride)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # warm-up outside the capture, as torch asks
        dm.encode_jpeg_batch(Y, Cc, quant, dims, restart=2, stride=stride, out=out, scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dm.encode_jpeg_batch(Y, Cc, quant, dims, restart=2, stride=stride, out=out, scratch=scratch)
    for k in (1, 0, 1):
        for dst, src in zip((Y, Cc, quant), sets[k]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        nb = eager[k][1].tolist()
        assert out[1].tolist() == nb and out[2].tolist() == [0, 0]
        for i in range(2):
            assert torch.equal(out[0][i, :nb[i]], eager[k][0][i, :nb[i]])
