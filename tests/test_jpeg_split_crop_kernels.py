"""The split device JPEG decode for crop boxes (include/rgbnm.h: rgbnm_jpeg_decode_batch_split_crop; csrc/jpeg_decode.hip:
split_verify_crop_kernel, split_write_crop_kernel, decode_crop_rest_kernel) against references that are not the code under test: the
box cut in torch out of the plain whole-grid decode of the same plan (held bit for bit against libjpeg by
tests/test_jpeg_decode_kernels.py), `path` against jpeg_split_ref.predict, `seg_live` and `walked` against the numpy restatement of
tests/jpeg_split_crop_ref.py.  The packed outputs lie in guarded buffers (tests/kernel_check.py): every element of the used prefix is
rewritten, nothing beyond it changes.  tests/test_jpeg_split_crop_cpu.py asserts, without a GPU, that every (file set, setting, box)
used here has an image that the segment lanes write, and live and skipped segments."""
import functools

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import jpeg_crop_ref as CR
import jpeg_split_crop_ref as XR
import jpeg_split_ref as SR
import kernel_check as KC
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu

EBOX = -26
BOX_NAMES = list(CR.boxes_for((8, 8)))


@pytest.fixture(params=XR.SETTINGS, ids=["seg256", "seg1024"])
def setting(request):
    sb, ms = request.param
    L.set_option("jpeg_min_seg", ms)
    yield sb, (ms or SR.MIN_SEG)
    L.set_option("jpeg_min_seg", 0)


class Set:
    """One batch of same-grid files: its plan on the device and the plain whole-grid decode of that plan (bits and status), computed
    once and left unchanged."""

    def __init__(self, files, grid):
        self.files, self.grid, self.n = files, grid, len(files)
        self.plan = dm.prepare_jpeg_batch(files, grid=grid)
        self.dev = dm.upload_jpeg_plan(self.plan, "cuda")
        Y, C, Q, st = dm.decode_jpeg_batch(self.plan, "cuda")
        torch.cuda.synchronize()
        self.Y, self.C, self.Q, self.status = Y.cpu(), C.cpu(), Q.cpu(), st.cpu()
        self.host_ok = [int(v) == 0 for v in self.plan.status[:self.n]]

    @functools.lru_cache(maxsize=None)
    def recs(self, sb, min_seg, rounds):
        return XR.records(self.plan, sb, rounds, min_seg, check=self.plan.nruns < 1000)

    def mixed(self):
        b = list(CR.boxes_for(self.grid).values())
        return [b[i % len(b)] for i in range(self.n)]


@functools.lru_cache(maxsize=None)
def sets(name):
    if name == "damaged":
        return Set(*XR.damaged_set())
    return Set(*XR.file_sets()[name])


class Call:
    """One call into guarded packed buffers."""

    def __init__(self, S, boxes, sb, rounds, offsets=None, ny=None, ncc=None):
        self.bx = torch.tensor(boxes, dtype=torch.int32)
        self.y_off, self.c_off, self.ny, self.ncc = dm.packed_offsets(self.bx) if offsets is None else (*offsets, ny, ncc)
        self.gy, self.gc = KC.guarded(self.ny, None, torch.int16), KC.guarded(self.ncc, None, torch.int16)
        self.Q, self.st = S.dev[4].clone(), S.dev[5].clone()
        self.gp = KC.guarded(S.n, None, torch.int32)
        self.wk = torch.full((S.plan.nruns,), -1, dtype=torch.int32, device="cuda")
        self.lv = torch.full((S.plan.nruns,), -1, dtype=torch.int32, device="cuda")
        self.args = (S.plan, S.dev, (self.gy.t, self.gc.t, self.Q, self.st), self.bx.cuda(), (self.y_off.cuda(), self.c_off.cuda(), self.ny, self.ncc))
        self.kw = dict(path=self.gp.t, seg_bits=sb, rounds=rounds, walked=self.wk, seg_live=self.lv)

    def launch(self):
        dm.launch_jpeg_split_crop(*self.args, **self.kw)
        torch.cuda.synchronize()
        return self


def check(S, c, boxes, setting, rounds, where, written=True):
    """Guards, (a) against the cut of the whole decode, (b) to (d), path, seg_live and walked against the restatement.  Returns (path, seg_live)."""
    sb, min_seg = setting
    c.gy.check(f"{where} Ypacked", written=written)
    c.gc.check(f"{where} Cpacked", written=written)
    c.gp.check(f"{where} path")
    Yp, Cp = c.gy.t.cpu(), c.gc.t.cpu()
    wantY, wantC = CR.cut(S.Y, S.C, boxes)
    st, path = c.st.cpu().tolist(), c.gp.t.tolist()
    for i, (t, l, h, w) in enumerate(boxes):
        if not S.host_ok[i]:
            continue
        ys, cs = slice(int(c.y_off[i]), int(c.y_off[i]) + 64 * h * w), slice(int(c.c_off[i]), int(c.c_off[i]) + 128 * (h // 2) * (w // 2))
        assert torch.equal(Yp[ys], wantY[ys]), (where, i, "Y against the whole-grid decode")
        assert torch.equal(Cp[cs], wantC[cs]), (where, i, "CbCr against the whole-grid decode")
        whole = int(S.status[i])
        assert whole <= st[i] <= 0, (where, i, "(b)", whole, st[i])
        assert whole != 0 or st[i] == 0, (where, i, "(c)")
        assert path[i] != 1 or st[i] == whole, (where, i, "(d)", whole, st[i])
    assert torch.equal(c.Q.cpu(), S.Q), (where, "quant")
    recs = S.recs(sb, min_seg, rounds)
    assert path == recs[0], (where, "path", path, recs[0])
    live, walked = XR.expected(S.plan, recs, boxes)
    got = c.lv.cpu().numpy()
    assert np.array_equal(got, live), (where, "seg_live", np.nonzero(got != live)[0][:8].tolist(), got[got != live][:8], live[got != live][:8])
    got = c.wk.cpu().numpy()
    assert np.array_equal(got, walked), (where, "walked", np.nonzero(got != walked)[0][:8].tolist(), got[got != walked][:8], walked[got != walked][:8])
    return path, live


@pytest.mark.parametrize("box", BOX_NAMES)
@pytest.mark.parametrize("name", ["pillow", "small", "padding", "tables", "many"])
def test_boxes(name, box, setting):
    """Every box of the list on every file of the set.  Well-formed files: status 0 everywhere."""
    S = sets(name)
    assert S.plan.nbad == 0 and not S.status.any()
    sb, min_seg = setting
    rounds = XR.rounds_for(S.plan, sb, min_seg)
    boxes = [CR.boxes_for(S.grid)[box]] * S.n
    c = Call(S, boxes, sb, rounds).launch()
    path, live = check(S, c, boxes, setting, rounds, f"{name} {box}")
    assert c.st.tolist() == [0] * S.n
    assert 1 in path and live.sum() > 0
    for i, data in enumerate(S.files):                          # a one-component file: an all-zero chroma crop
        if dm.read_coefficients_bytes(data)[3] is None:
            t, l, h, w = boxes[i]
            assert not c.gc.t[int(c.c_off[i]):int(c.c_off[i]) + 128 * (h // 2) * (w // 2)].any(), (name, box, i)


@pytest.mark.parametrize("rounds", [0, 1, None])
def test_damaged_runs_and_few_rounds_fall_back_where_the_restatement_says(rounds, setting):
    """Files whose scan no longer decodes beside well-formed ones, a box of its own per file: the same box bits as the whole decode
    (zeros behind an error included), the status between the whole decode's and 0, and the whole decode's where path is 1."""
    S = sets("damaged")
    sb, min_seg = setting
    assert S.plan.nbad == 0 and int((S.status < 0).sum()) >= 4      # the one-lane walk of the damaged files ends in an error
    r = XR.rounds_for(S.plan, sb, min_seg) if rounds is None else rounds
    boxes = S.mixed()
    c = Call(S, boxes, sb, r).launch()
    path, _ = check(S, c, boxes, setting, r, f"damaged, rounds {r}")
    assert 2 in path and all(p != 1 for p, s in zip(path, S.status.tolist()) if s < 0)
    if rounds is None:
        assert 1 in path


@functools.lru_cache(maxsize=None)
def mixed_set():
    """Grid (8, 8): marker-less files, files with a marker per MCU row, a gray one, and a file with one scan per component, which the
    device refuses."""
    files = [JC.encode(JC.noisy(64, 64, 21), quality=92), JC.encode(JC.noisy(64, 64, 22), quality=85, restart_marker_rows=1),
             JC.encode(JC.noisy(64, 64, 23, gray=True), quality=95), JC.three_scans().data, JC.encode(JC.noisy(64, 64, 25), quality=97),
             JC.encode(JC.noisy(64, 64, 24), quality=95, restart_marker_rows=1)]
    return Set(files, (8, 8)), 3


def test_mixed_batch_with_a_refused_file_and_one_bad_box(setting):
    S, refused = mixed_set()
    sb, min_seg = setting
    assert S.plan.nbad == 1 and S.plan.status[refused] < 0
    rounds = XR.rounds_for(S.plan, sb, min_seg)
    good = S.mixed()
    bx = torch.tensor(good, dtype=torch.int32)
    y_off, c_off, ny, ncc = dm.packed_offsets(bx)
    canary = torch.tensor(KC.CANARY[2], dtype=torch.int16)
    for bad_i, (what, box, yo) in enumerate([("odd", (1, 2, 2, 2), None), ("outside", (0, 0, 10, 8), None), ("offset past y_elems", None, ny - 64),
                                             ("misaligned offset", None, 4)]):
        i = (0, 4, 1, 2)[bad_i]                                  # split and written by segment lanes, split, restart runs, gray
        b, yoff = bx.clone(), y_off.clone()
        if box is not None:
            b[i] = torch.tensor(box, dtype=torch.int32)
        if yo is not None:
            yoff[i] = yo
        c = Call(S, b.tolist(), sb, rounds, offsets=(yoff, c_off), ny=ny, ncc=ncc).launch()
        c.gy.check(f"bad box ({what}) Ypacked", written=False)
        c.gc.check(f"bad box ({what}) Cpacked", written=False)
        st = c.st.tolist()
        assert st == [EBOX if k == i else int(S.plan.status[k]) for k in range(S.n)], (what, st)
        recs = S.recs(sb, min_seg, rounds)
        assert c.gp.t.tolist() == recs[0] and recs[0][refused] == 0 and recs[0][0] == recs[0][4] == 1      # a bad box does not change the path
        Yp, Cp = c.gy.t.cpu(), c.gc.t.cpu()
        wantY, wantC = CR.cut(S.Y, S.C, bx)
        for k in range(S.n):
            ys = slice(int(y_off[k]), int(y_off[k]) + 64 * good[k][2] * good[k][3])
            cs = slice(int(c_off[k]), int(c_off[k]) + 128 * (good[k][2] // 2) * (good[k][3] // 2))
            if k in (i, refused):
                assert bool((Yp[ys] == canary).all()) and bool((Cp[cs] == canary).all()), (what, k, "a refused image's slots were written")
            else:
                assert torch.equal(Yp[ys], wantY[ys]) and torch.equal(Cp[cs], wantC[cs]), (what, k)
        live, walked = XR.expected(S.plan, recs, good)
        mine = S.plan.runs[:S.plan.nruns, 2].numpy() == i
        live[mine], walked[mine] = 0, 0
        assert np.array_equal(c.lv.cpu().numpy(), live) and np.array_equal(c.wk.cpu().numpy(), walked), what


@pytest.fixture(params=[(1, 1), (1, 64), (0, 1), (0, 64)], ids=["wgs1_lanes1", "wgs1_lanes64", "lanes1", "lanes64"])
def grids(request):
    wgs, lanes = request.param
    L.set_option("jpeg_split_wgs", wgs)
    L.set_option("jpeg_lanes", lanes)
    yield request.param
    L.set_option("jpeg_split_wgs", 0)
    L.set_option("jpeg_lanes", 0)


@pytest.mark.parametrize("name", ["pillow", "small"])
def test_one_workgroup_and_1_or_64_lanes_give_the_same_bits(name, grids, setting):
    """Option jpeg_split_wgs = 1: every grid-stride loop goes round again, the loop over the list of live slots included (more live
    segments than one wave's lanes).  All against the same references, so the same bits."""
    S = sets(name)
    sb, min_seg = setting
    rounds = XR.rounds_for(S.plan, sb, min_seg)
    boxes = [CR.boxes_for(S.grid)["largest"]] * S.n if name == "pillow" else S.mixed()
    c = Call(S, boxes, sb, rounds).launch()
    _, live = check(S, c, boxes, setting, rounds, f"{name} {grids}")
    if name == "pillow":
        assert live.sum() > 64, "the list is no longer than one wave"


def test_live_segments_behind_two_table_sets_share_a_wave():
    """A file behind the standard tables and one behind long tables of its own, 64 segments per wave: the live segments of both are
    neighbours in the list and fit one wave, so no table set serves that wave and the write pass reads the tables from global memory."""
    L.set_option("jpeg_min_seg", 2)
    L.set_option("jpeg_lanes", 64)
    try:
        S = Set([JC.standard_420(7, 96, 64, restart=0).data, JC.long_codes().data], (8, 12))
        rounds = XR.rounds_for(S.plan, 256, 2)
        boxes = [CR.boxes_for(S.grid)["mcu_column"], CR.boxes_for(S.grid)["mcu_row"]]
        c = Call(S, boxes, 256, rounds).launch()
        path, live = check(S, c, boxes, (256, 2), rounds, "two table sets")
        assert path == [1, 1] and S.plan.ntables > 4 and live[0] > 0 and live[1] > 0 and live.sum() <= 64
    finally:
        L.set_option("jpeg_min_seg", 0)
        L.set_option("jpeg_lanes", 0)


def test_two_calls_give_identical_bytes(setting):
    """The order of the runs in the list is the order of their atomic adds; the outputs do not depend on it."""
    S = sets("small")
    sb, min_seg = setting
    rounds = XR.rounds_for(S.plan, sb, min_seg)
    boxes = S.mixed()
    a, b = Call(S, boxes, sb, rounds).launch(), Call(S, boxes, sb, rounds).launch()
    check(S, a, boxes, setting, rounds, "first call")
    for x, y in ((a.gy.raw, b.gy.raw), (a.gc.raw, b.gc.raw), (a.st, b.st), (a.gp.raw, b.gp.raw), (a.wk, b.wk), (a.lv, b.lv)):
        assert torch.equal(x, y)


def test_graph_capture_then_replay_with_other_boxes_and_other_files(setting):
    """One capture; the boxes, the offsets and the plan's device buffers are refilled -- the same files in the opposite order, which
    gives as many runs, tables and stream bytes -- and every replay equals the references of what it was fed."""
    sb, min_seg = setting
    files = [JC.encode(JC.noisy(64, 64, 40 + i, gray=(i == 2)), quality=90 + i, **({"restart_marker_rows": 1} if i == 3 else {})) for i in range(5)]
    A, B = Set(files, (8, 8)), Set(files[::-1], (8, 8))
    assert (A.plan.nruns, A.plan.ntables, A.plan.stream_bytes) == (B.plan.nruns, B.plan.ntables, B.plan.stream_bytes)
    rounds = max(XR.rounds_for(S.plan, sb, min_seg) for S in (A, B))
    names = list(CR.boxes_for((8, 8)))
    feeds = [(S, [CR.boxes_for((8, 8))[names[(i + k) % len(names)]] for i in range(S.n)]) for k, S in ((1, B), (4, A), (6, B), (0, A))]
    offs = [dm.packed_offsets(torch.tensor(bx, dtype=torch.int32)) for _, bx in feeds]
    ny, ncc = max(o[2] for o in offs), max(o[3] for o in offs)
    dev = [t.clone() for t in A.dev]
    cap = Set.__new__(Set)                                      # the captured call's view: A's plan sizes, device buffers of its own
    cap.plan, cap.dev, cap.n = A.plan, dev, A.n
    c = Call(cap, feeds[3][1], sb, rounds, offsets=offs[3][:2], ny=ny, ncc=ncc)
    c.kw["scratch"] = dm.jpeg_split_crop_scratch(A.plan, sb)
    bdev, (yo, co, _, _) = c.args[3], c.args[4]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture, as torch asks
        dm.launch_jpeg_split_crop(*c.args, **c.kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dm.launch_jpeg_split_crop(*c.args, **c.kw)
    canary = torch.tensor(KC.CANARY[2], dtype=torch.int16)
    for (S, boxes), off in zip(feeds, offs):
        for d, h in zip(dev, S.plan.buffers()):
            d[:h.shape[0]].copy_(h)
        c.Q.copy_(dev[4])
        c.st.copy_(dev[5])
        bdev.copy_(torch.tensor(boxes, dtype=torch.int32))
        yo.copy_(off[0])
        co.copy_(off[1])
        c.y_off, c.c_off = off[0], off[1]
        c.gy.t.fill_(KC.CANARY[2])
        c.gc.t.fill_(KC.CANARY[2])
        c.wk.fill_(-1)
        c.lv.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(S, c, boxes, setting, rounds, "replay", written=False)
        assert bool((c.gy.t.cpu()[off[2]:] == canary).all()) and bool((c.gc.t.cpu()[off[3]:] == canary).all())
        assert not (c.gy.t[:off[2]] == canary).any() and not (c.gc.t[:off[3]] == canary).any()
        assert c.st.tolist() == [0] * S.n
    del graph


def test_python_entries_and_defaults():
    """decode_jpeg_batch_split_crop with the default seg_bits and rounds and read_coefficients_batch_crop_device(split=True) against
    the host crop reader's bits."""
    data = [JC.encode(JC.noisy(128, 128, 21 + i), quality=95) for i in range(2)]          # 16 segments of the default size and more
    plan = dm.prepare_jpeg_batch(data, grid=(16, 16))
    boxes = [[2, 4, 8, 6], [0, 0, 16, 16]]
    Y, C, Q, st = dm.decode_jpeg_batch(plan, "cuda")
    wantY, wantC = CR.cut(Y.cpu(), C.cpu(), boxes)
    Yp, Cp, Q2, st2, yo, co, path = dm.decode_jpeg_batch_split_crop(plan, "cuda", boxes=boxes, return_path=True)
    assert len(dm.decode_jpeg_batch_split_crop(plan, "cuda", boxes=boxes)) == 6
    assert path.tolist() == SR.predict(plan, dm.JPEG_SPLIT_SEG_BITS, dm.JPEG_SPLIT_ROUNDS)[0] == [1, 1] and st2.tolist() == [0, 0]
    assert torch.equal(Yp.cpu(), wantY) and torch.equal(Cp.cpu(), wantC) and torch.equal(Q2, Q) and yo.dtype == co.dtype == torch.int64
    Y3, C3, Q3, yo3, co3 = dm.read_coefficients_batch_crop_device(data, boxes, grid=(16, 16), device="cuda", split=True)
    assert torch.equal(Y3.cpu(), wantY) and torch.equal(C3.cpu(), wantC) and torch.equal(Q3, Q) and torch.equal(yo3, yo) and torch.equal(co3, co)
    with pytest.raises(ValueError, match="not even"):
        dm.read_coefficients_batch_crop_device(data, [[0, 0, 16, 16], [1, 0, 2, 2]], grid=(16, 16), device="cuda", split=True)


def test_loader_with_crop_split_yields_the_crop_on_host_tensors(tmp_path):
    """Marker-less 512 x 512 files, one gray and one progressive (the device refuses it: decoded by the host reader and cut to its
    box): the batch tensors, labels and drawn parameters of crop_on_host=True at the same seed and epoch, bit for bit."""
    from PIL import Image

    import rgb_no_more_amd as rg
    from rgb_no_more_amd.loader import DCTBatchLoader
    paths = []
    for i in range(8):
        img = JC.noisy(512, 512, 80 + i, gray=(i == 5))
        p = tmp_path / f"s{i}.jpg"
        if i == 2:
            Image.fromarray(img).save(str(p), quality=90, subsampling="4:2:0", progressive=True)
        else:
            p.write_bytes(JC.encode(img, quality=90))
        paths.append(str(p))
    labels = list(range(10, 18))
    tr = rg.datasets.get_transform("imagenet_dct", "train", ops_list=CT.VITTI_OPS, ops_magnitude=3, dtype=torch.float32, fused=True)
    kw = dict(batch_size=4, device="cuda", threads=4, prefetch=2, shuffle=True, seed=7, transform=tr)

    def batches(loader, epoch):
        loader.set_epoch(epoch)
        out = []
        for (Y, C), lab in loader:
            packed, nops = loader.last_packed
            out.append((Y.clone(), C.clone(), lab.clone(), packed.copy(), nops))
        return out

    host = DCTBatchLoader(paths, labels, crop_on_host=True, **kw)
    dev = DCTBatchLoader(paths, labels, decode="device", crop_on_device="split", **kw)
    assert dev.crop_on_device is True and dev.crop_split is True and dev.jpeg_split is False and host.crop_split is False
    a, b = batches(host, 3), batches(dev, 3)
    assert len(a) == len(b) == 2
    for (Yh, Ch, lh, ph, nh), (Yd, Cd, l_d, pd, nd) in zip(a, b):
        assert Yd.is_cuda and tuple(Yd.shape)[:2] == (4, 1)
        assert torch.equal(lh, l_d) and nh == nd and ph.tobytes() == pd.tobytes()
        assert torch.equal(Yh, Yd) and torch.equal(Ch, Cd)
    # the files are long enough for the default segment size to split them
    plan = dm.prepare_jpeg_batch([paths[0], paths[5]], grid=(64, 64))
    assert SR.predict(plan, dm.JPEG_SPLIT_SEG_BITS, 0)[0] == [2, 2], "a file of the folder is too short to be split"
