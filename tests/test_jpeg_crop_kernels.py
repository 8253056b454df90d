"""The crop form of the device JPEG decode (csrc/jpeg_decode.hip, decode_crop_kernel; include/rgbnm.h, rgbnm_jpeg_decode_batch_crop)
against two references that are not the code under test: the box cut in torch out of the whole-grid decode of the same plan (held bit
for bit against libjpeg by tests/test_jpeg_decode_kernels.py), and the host libjpeg crop reader.  The packed outputs lie in guarded
buffers (tests/kernel_check.py): every element of the used prefix is rewritten, nothing beyond it changes.  The `walked` array shows
that runs outside a box are skipped, not merely masked, and that the others stop early (tests/jpeg_crop_ref.py restates the count).
Well-formed files only: damaged streams are exercised on the CPU (tools/jpeg_crop_check.cpp runs the same walk under sanitizers)."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import jpeg_crop_ref as CR
import kernel_check as KC
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu

EBOX = -26


@pytest.fixture(scope="module", autouse=True)
def jpeg_dir(tmp_path_factory):
    """The host crop reader takes paths: the files of a set are written here once."""
    Set.dir = str(tmp_path_factory.mktemp("jpeg_crop"))
    yield Set.dir
    sets.cache_clear()


class Set:
    """One batch of same-grid files: its plan on the device and the whole-grid decode of that plan, computed once and left unchanged."""
    dir = None

    def __init__(self, name, files, grid, gray=()):
        self.name, self.files, self.grid, self.gray, self.n = name, files, grid, gray, len(files)
        self.paths = []
        for data in files:
            p = os.path.join(Set.dir, hashlib.sha1(data).hexdigest() + ".jpg")
            if not os.path.exists(p):
                with open(p, "wb") as fh:
                    fh.write(data)
            self.paths.append(p)
        self.plan = dm.prepare_jpeg_batch(files, grid=grid)
        assert self.plan.nbad == 0, self.plan.messages
        self.dev = dm.upload_jpeg_plan(self.plan, "cuda")
        Y, C, Q, st = dm.decode_jpeg_batch(self.plan, "cuda")
        torch.cuda.synchronize()
        assert st.tolist() == [0] * self.n
        self.Y, self.C, self.Q = Y.cpu(), C.cpu(), Q.cpu()

    def mixed(self):
        """File i takes box i of the list, round and round: neighbouring lanes skip, stop early and walk to the end."""
        b = list(CR.boxes_for(self.grid).values())
        return [b[i % len(b)] for i in range(self.n)]


@functools.lru_cache(maxsize=None)
def sets(name):
    p = JC.pillow_files()
    if name == "pillow":        # grid (9, 13), odd on both sides: 1 run, one per MCU, per 2 and 3 MCUs, per MCU row, gray, own tables
        keys = ("q75", "rst_blocks1", "rst_blocks2", "rst_rows1", "gray_rst", "optimize", "q100", "rst_blocks3")
        return Set(name, [p[k] for k in keys], (9, 13), gray=(4,))
    if name == "sweep":         # grid (11, 13): 1, 42 and 11 runs; run boundaries inside MCU rows, runs crossing rows
        return Set(name, [s.data for s in JC.sweep()], (11, 13))
    if name == "tables":        # grid (8, 12), 4 x 6 MCUs: six distinct tables beside the standard four (no wave can share them);
        std = [JC.standard_420(40 + k, w=96, h=64, restart=r).data for k, r in enumerate((1, 6, 0))]      # one run per MCU, per MCU row, one
        return Set(name, [JC.long_codes().data] + std, (8, 12))
    if name == "many":          # grid (5, 7): 241 files, 8275 runs
        m = JC.many_runs()
        return Set(name, [s.data for s in m], (5, 7), gray=tuple(i for i, s in enumerate(m) if s.C is None))
    raise KeyError(name)


def crop_and_compare(S, boxes, where, expect_skip=True, expect_early=True):
    bx = torch.tensor(boxes, dtype=torch.int32)
    y_off, c_off, ny, ncc = dm.packed_offsets(bx)
    gy, gc = KC.guarded(ny, None, torch.int16), KC.guarded(ncc, None, torch.int16)
    Q, st = S.dev[4].clone(), S.dev[5].clone()
    wk = torch.full((S.plan.nruns,), -1, dtype=torch.int32, device="cuda")
    got_off = dm.launch_jpeg_decode(S.plan, S.dev, (gy.t, gc.t, Q, st), boxes=bx, walked=wk)
    torch.cuda.synchronize()
    gy.check(f"{where} Ypacked")                                # every element rewritten, the guard bands untouched
    gc.check(f"{where} Cpacked")
    assert st.tolist() == [0] * S.n, (where, st.tolist())
    assert torch.equal(got_off[0].cpu(), y_off) and torch.equal(got_off[1].cpu(), c_off)
    Yp, Cp = gy.t.cpu(), gc.t.cpu()
    wantY, wantC = CR.cut(S.Y, S.C, bx)                          # the box cut out of the whole-grid device decode of the same plan
    assert torch.equal(Yp, wantY), (where, "Y against the whole-grid decode")
    assert torch.equal(Cp, wantC), (where, "CbCr against the whole-grid decode")
    hY, hC, hQ, hyo, hco = dm.read_coefficients_batch_crop(S.paths, bx, grid=S.grid)      # the host libjpeg path
    assert torch.equal(hyo, y_off) and torch.equal(hco, c_off)
    assert torch.equal(Yp, hY), (where, "Y against the host crop reader")
    assert torch.equal(Cp, hC), (where, "CbCr against the host crop reader")
    assert torch.equal(Q.cpu(), hQ), (where, "quant")
    for i in S.gray:                                             # a one-component file: an all-zero chroma crop
        t, l, h, w = boxes[i]
        assert not Cp[int(c_off[i]):int(c_off[i]) + 2 * (h // 2) * (w // 2) * 64].any(), (where, i)
    want = CR.plan_walked(S.plan, boxes)
    got = wk.cpu().numpy()
    assert np.array_equal(got, want), (where, "walked", np.nonzero(got != want)[0][:8].tolist(), got[got != want][:8], want[got != want][:8])
    nmcu = S.plan.runs[:S.plan.nruns, 4].numpy()
    if expect_skip:
        assert (got == 0).any(), (where, "no run was skipped")
    if expect_early:
        assert ((got > 0) & (got < nmcu)).any(), (where, "no run stopped early")
    return Yp, Cp, got


BOX_NAMES = list(CR.boxes_for((8, 8)))


@pytest.mark.parametrize("box", BOX_NAMES + ["mixed"])
@pytest.mark.parametrize("name", ["pillow", "sweep", "tables"])
def test_boxes(name, box):
    """Every box of the list on every file of the set, then the batch that mixes them.  On the odd grids the largest box ends at the
    last even row and column: the padding blocks, and on (9, 13) the grid's last row and column, fall outside it."""
    S = sets(name)
    boxes = S.mixed() if box == "mixed" else [CR.boxes_for(S.grid)[box]] * S.n
    # the largest box of the even (8, 12) grid needs every MCU: nothing to skip there; a box that holds the grid's last MCU lets no
    # run stop early
    _, _, walked = crop_and_compare(S, boxes, f"{name} {box}", expect_skip=not (name == "tables" and box == "largest"),
                                    expect_early=box in ("mixed", "top_left", "top_right", "middle", "mcu_row"))
    nmcu = S.plan.runs[:S.plan.nruns, 4].numpy()
    if name == "tables" and box == "largest":
        assert np.array_equal(walked, nmcu)
    if name == "sweep" and box == "top_left":                    # 1, 42 and 11 runs: each file walks its first MCU and no other
        assert walked.tolist() == [1] + [1] + [0] * 41 + [1] + [0] * 10


@pytest.fixture
def lanes(request):
    L.set_option("jpeg_lanes", request.param)
    yield request.param
    L.set_option("jpeg_lanes", 0)


@pytest.mark.parametrize("lanes", [1, 64], indirect=True)
@pytest.mark.parametrize("name", ["pillow", "sweep", "tables", "many"])
def test_runs_per_wave_1_and_64_give_the_same_bits(name, lanes):
    """Both against the same references, so the same bits.  "many" with one run per wave: 8275 workgroups' worth of runs on a grid
    capped at 4096, so the grid-stride loop goes round more than once; with 64 per wave, waves whose lanes belong to different files
    and table families, most of them skipped."""
    S = sets(name)
    crop_and_compare(S, S.mixed(), f"{name} mixed, {lanes} runs per wave")
    if name == "many":
        assert S.plan.nruns == 8275 and S.n == 241


def test_one_bad_box_fails_its_image_alone():
    """An odd box, a box outside the grid and an offset past y_elems, one image each: RGBNM_JPEG_EBOX for that image, its slots
    untouched, nothing walked for it; the other images are correct."""
    S = sets("pillow")
    good = S.mixed()
    bx = torch.tensor(good, dtype=torch.int32)
    y_off, c_off, ny, ncc = dm.packed_offsets(bx)
    for bad_i, (what, box, yo) in enumerate([("odd", (1, 2, 2, 2), None), ("outside", (0, 0, 10, 12), None), ("outside", (4, 12, 2, 2), None),
                                             ("negative", (-2, 0, 2, 2), None), ("empty", (2, 2, 0, 2), None),
                                             ("offset past y_elems", None, ny - 64), ("misaligned offset", None, 4)]):
        i = (bad_i * 3 + 1) % S.n
        b, yoff = bx.clone(), y_off.clone()
        if box is not None:
            b[i] = torch.tensor(box, dtype=torch.int32)
        if yo is not None:
            yoff[i] = yo + (0 if yo < 8 else int(y_off[i]) % 8)
            if yo >= 8:
                assert int(yoff[i]) + 64 * good[i][2] * good[i][3] > ny
        gy, gc = KC.guarded(ny, None, torch.int16), KC.guarded(ncc, None, torch.int16)
        Q, st = S.dev[4].clone(), S.dev[5].clone()
        wk = torch.full((S.plan.nruns,), -1, dtype=torch.int32, device="cuda")
        dm.launch_jpeg_decode(S.plan, S.dev, (gy.t, gc.t, Q, st), boxes=b.cuda(), packed_out=(yoff.cuda(), c_off.cuda(), ny, ncc), walked=wk)
        torch.cuda.synchronize()
        gy.check(f"bad box ({what}) Ypacked", written=False)
        gc.check(f"bad box ({what}) Cpacked", written=False)
        assert st.tolist() == [EBOX if k == i else 0 for k in range(S.n)], (what, st.tolist())
        Yp, Cp = gy.t.cpu(), gc.t.cpu()
        wantY, wantC = CR.cut(S.Y, S.C, bx)
        canary = torch.tensor(KC.CANARY[2], dtype=torch.int16)
        for k in range(S.n):
            ys = slice(int(y_off[k]), int(y_off[k]) + 64 * good[k][2] * good[k][3])
            cs = slice(int(c_off[k]), int(c_off[k]) + 128 * (good[k][2] // 2) * (good[k][3] // 2))
            if k == i:
                assert bool((Yp[ys] == canary).all()) and bool((Cp[cs] == canary).all()), (what, "the refused image's slots were written")
            else:
                assert torch.equal(Yp[ys], wantY[ys]) and torch.equal(Cp[cs], wantC[cs]), (what, k)
        want = CR.plan_walked(S.plan, good)
        want[S.plan.runs[:S.plan.nruns, 2].numpy() == i] = 0
        assert np.array_equal(wk.cpu().numpy(), want), what


def test_captured_call_reads_the_boxes_at_replay():
    """Captured once in a HIP graph; replayed after new boxes and offsets were copied into the same device arrays."""
    S = sets("sweep")
    names = list(CR.boxes_for(S.grid))
    A = S.mixed()
    B = [CR.boxes_for(S.grid)[names[(i + 3) % len(names)]] for i in range(S.n)]
    Cc = [CR.boxes_for(S.grid)["largest"]] * S.n
    offs = {k: dm.packed_offsets(torch.tensor(v, dtype=torch.int32)) for k, v in (("A", A), ("B", B), ("C", Cc))}
    ny, ncc = max(o[2] for o in offs.values()), max(o[3] for o in offs.values())
    gy, gc = KC.guarded(ny, None, torch.int16), KC.guarded(ncc, None, torch.int16)
    Q, st = S.dev[4].clone(), S.dev[5].clone()
    wk = torch.zeros(S.plan.nruns, dtype=torch.int32, device="cuda")
    bdev = torch.tensor(A, dtype=torch.int32, device="cuda")
    yo, co = offs["A"][0].cuda(), offs["A"][1].cuda()
    ws = torch.cuda.Stream()
    ws.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ws):
        dm.launch_jpeg_decode(S.plan, S.dev, (gy.t, gc.t, Q, st), boxes=bdev, packed_out=(yo, co, ny, ncc), walked=wk)      # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=ws):
        dm.launch_jpeg_decode(S.plan, S.dev, (gy.t, gc.t, Q, st), boxes=bdev, packed_out=(yo, co, ny, ncc), walked=wk)
    for key, boxes in (("B", B), ("C", Cc), ("A", A)):
        bdev.copy_(torch.tensor(boxes, dtype=torch.int32))
        yo.copy_(offs[key][0])
        co.copy_(offs[key][1])
        gy.t.fill_(KC.CANARY[2])
        gc.t.fill_(KC.CANARY[2])
        wk.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        gy.check(f"replay {key} Ypacked", written=False)
        gc.check(f"replay {key} Cpacked", written=False)
        wantY, wantC = CR.cut(S.Y, S.C, boxes)
        assert torch.equal(gy.t.cpu()[:offs[key][2]], wantY) and torch.equal(gc.t.cpu()[:offs[key][3]], wantC), key
        canary = torch.tensor(KC.CANARY[2], dtype=torch.int16)
        assert bool((gy.t.cpu()[offs[key][2]:] == canary).all()) and bool((gc.t.cpu()[offs[key][3]:] == canary).all()), key
        assert np.array_equal(wk.cpu().numpy(), CR.plan_walked(S.plan, boxes)), key
        assert st.tolist() == [0] * S.n
    del g


@pytest.mark.parametrize("name", ["pillow", "sweep", "tables"])
def test_plain_call_on_the_same_plans_gives_the_host_readers_bits(name):
    """The whole-grid call is what it was: against the host reader, not against a saved copy of itself."""
    S = sets(name)
    hb, wb = S.grid
    for i, data in enumerate(S.files):
        _, quant, Yh, Ch = dm.read_coefficients_bytes(data)
        if Ch is None:
            Ch = torch.zeros((2, (hb + 1) // 2, (wb + 1) // 2, 8, 8), dtype=torch.int16)
        q = torch.ones((3, 8, 8), dtype=torch.int16)
        q[:quant.shape[0]] = quant
        assert torch.equal(S.Y[i], Yh) and torch.equal(S.C[i], Ch) and torch.equal(S.Q[i], q), (name, i)


def test_python_entries():
    """decode_jpeg_batch(boxes=...) and the raising convenience form against the host crop reader."""
    S = sets("pillow")
    boxes = S.mixed()
    hY, hC, hQ, hyo, hco = dm.read_coefficients_batch_crop(S.paths, boxes, grid=S.grid)
    Yp, Cp, Q, st, yo, co = dm.decode_jpeg_batch(S.plan, "cuda", boxes=boxes)
    assert Yp.is_cuda and yo.is_cuda and yo.dtype == torch.int64 and co.dtype == torch.int64 and Yp.dim() == 1 and Cp.dim() == 1
    assert torch.equal(Yp.cpu(), hY) and torch.equal(Cp.cpu(), hC) and torch.equal(Q.cpu(), hQ) and st.tolist() == [0] * S.n
    assert torch.equal(yo.cpu(), hyo) and torch.equal(co.cpu(), hco)
    Yp, Cp, Q, yo, co = dm.read_coefficients_batch_crop_device(S.files, np.asarray(boxes), grid=S.grid, device="cuda")
    assert torch.equal(Yp.cpu(), hY) and torch.equal(Cp.cpu(), hC) and torch.equal(Q.cpu(), hQ) and torch.equal(yo.cpu(), hyo)
    with pytest.raises(dm.libjpeg_exception, match="bytes #1"):
        dm.read_coefficients_batch_crop_device([S.files[0], JC.g1_files()["c64x64"]], boxes[:2], grid=S.grid, device="cuda")
    with pytest.raises(ValueError, match="not even"):
        dm.read_coefficients_batch_crop_device(S.files[:1], [[0, 0, 10, 12]], grid=S.grid, device="cuda")
