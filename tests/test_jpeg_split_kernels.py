"""The split device JPEG decode (csrc/jpeg_split.h, jpeg_decode.hip: one lane per bit segment of a run) against the host libjpeg
reader AND the plain device call on the same plan, bit for bit, into guarded outputs; `path` against the plain-Python restatement
of the scheme (tests/jpeg_split_ref.py).  Well-formed files only: damaged streams are exercised on the CPU
(tools/jpeg_split_check.cpp runs the same segment walk under sanitizers).

Two settings run every file set: seg_bits 256 with the default threshold (runs of at least 16 segments are split: 481 bytes), and
seg_bits 1024 with option "jpeg_min_seg" = 2, so that files of one or two KB are split there too.  rounds is at most 64, so
convergence is CERTAIN (rounds >= segments - 1) for runs of up to 2080 bytes at 256 bits and 8320 bytes at 1024; where a test says
`certain`, it asserts that the files are that small and that every split image reports path 1."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as JC
import jpeg_ref as JR
import jpeg_split_ref as SR
import jpeg_writer as JW
import kernel_check as KC
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu

SETTINGS = [(256, 0), (1024, 2)]                  # (seg_bits, option "jpeg_min_seg"; 0: the default, 16)


@pytest.fixture(params=SETTINGS, ids=["seg256", "seg1024"])
def setting(request):
    sb, ms = request.param
    L.set_option("jpeg_min_seg", ms)
    yield sb, (ms or SR.MIN_SEG)
    L.set_option("jpeg_min_seg", 0)


@functools.lru_cache(maxsize=None)
def host(data):
    _, quant, Y, CbCr = dm.read_coefficients_bytes(data)
    hb, wb = Y.shape[1:3]
    if CbCr is None:
        CbCr = torch.zeros((2, (hb + 1) // 2, (wb + 1) // 2, 8, 8), dtype=torch.int16)
    q = torch.ones((3, 8, 8), dtype=torch.int16)
    q[:quant.shape[0]] = quant
    return Y, CbCr, q


def grid_of(data):
    return tuple(host(data)[0].shape[1:3])


class Outputs:
    """Guarded Y / CbCr / quant / status / path for n files of one grid."""

    def __init__(self, n, grid):
        hb, wb = grid
        hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
        self.g = [KC.guarded(n * hb * wb, 64, torch.int16), KC.guarded(n * 2 * hbc * wbc, 64, torch.int16),
                  KC.guarded(n * 3, 64, torch.int16), KC.guarded(n, None, torch.int32), KC.guarded(n, None, torch.int32)]
        self.t = (self.g[0].t.view(n, 1, hb, wb, 8, 8), self.g[1].t.view(n, 2, hbc, wbc, 8, 8), self.g[2].t.view(n, 3, 8, 8), self.g[3].t)
        self.path = self.g[4].t

    def check(self, where, written=True, path=True):
        torch.cuda.synchronize()
        for g, name in zip(self.g[:4], ("Y", "CbCr", "quant", "status")):
            g.check(f"{where} {name}", written=written)
        if path:
            self.g[4].check(f"{where} path")


def run_split(plan, out, sb, rounds):
    """decode_jpeg_batch's steps with the split launch writing into the guarded path."""
    dev = dm.upload_jpeg_plan(plan, "cuda")
    out.t[2].copy_(dev[4])
    out.t[3].copy_(dev[5])
    dm.launch_jpeg_decode(plan, dev, out.t, split=True, seg_bits=sb, rounds=rounds, path=out.path)


def split_and_compare(files, grid, setting, rounds, where, certain=False):
    """Plain and split call on one plan: equal bits, equal to the host reader's, status zero, path as the restatement predicts.
    rounds None: as many as certain convergence needs (at most 64).  Returns (plan, path list)."""
    sb, min_seg = setting
    plan = dm.prepare_jpeg_batch(files, grid=grid)
    assert plan.nbad == 0, plan.messages
    _, longest, _ = SR.predict(plan, sb, 0, min_seg)
    if rounds is None:
        rounds = min(64, max(0, longest - 1))
    want, _, _ = SR.predict(plan, sb, rounds, min_seg)
    if certain:
        assert rounds >= longest - 1, (where, longest)
        assert all(p == 1 for p in want if p), (where, want)      # the restatement agrees with the contract
    a, b = Outputs(len(files), grid), Outputs(len(files), grid)
    dm.decode_jpeg_batch(plan, "cuda", out=a.t)
    a.check(where + " plain", path=False)
    run_split(plan, b, sb, rounds)
    b.check(where + " split")
    assert b.t[3].tolist() == [0] * len(files), (where, b.t[3].tolist())
    for x, y, name in zip(a.t, b.t, ("Y", "CbCr", "quant", "status")):
        assert torch.equal(x, y), (where, name, "split differs from the plain call")
    for i, data in enumerate(files):
        for got, ref, name in zip(b.t, host(data), ("Y", "CbCr", "quant")):
            assert torch.equal(got[i].cpu(), ref), (where, i, name, "split differs from the host reader")
    got = b.path.tolist()
    assert got == want, (where, "path", got, want)
    return plan, got


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def smooth(h, w, seed):
    small = np.random.default_rng(seed).integers(0, 256, (3, 3, 3), dtype=np.uint8)
    return np.asarray(Image.fromarray(small).resize((w, h), Image.BICUBIC))


@functools.lru_cache(maxsize=None)
def pillow_set():
    """name -> bytes: 4:2:0 smooth and noise, even and odd grids ((5, 3) and (5, 7): padding blocks dropped, chroma grid rounded
    up), one gray file.  Scans of 0.5 to 2 KB."""
    return {"smooth_8x8": JC.encode(smooth(64, 64, 1), quality=98), "noise_6x8": JC.encode(JC.noisy(48, 64, 3), quality=90),
            "noise_5x7": JC.encode(JC.noisy(37, 53, 4), quality=92), "noise_5x3": JC.encode(JC.noisy(40, 24, 6), quality=96),
            "smooth_5x3": JC.encode(smooth(40, 24, 2), quality=100), "gray_7x5": JC.encode(JC.noisy(56, 40, 5, gray=True), quality=92)}


def repack(data):
    """The file's kept coefficients written again as ONE run (no restart interval) behind the same tables; the MCU padding is zero."""
    f = JR.parse(data)
    Y, C, quant = JR.decode_file(data)
    nc = f["ncomp"]
    sampling = list(zip(f["hs"], f["vs"])) if nc == 3 else [(1, 1)]
    planes = []
    for kept, (gh, gw) in zip([Y] + ([C[0], C[1]] if nc == 3 else []), JW.padded_grids(f["width"], f["height"], sampling)):
        p = np.zeros((gh, gw, 64), np.int64)
        p[:kept.shape[0], :kept.shape[1]] = kept
        planes.append(p)
    tables = [(JW.bits_vals(f["dc"][c]), JW.bits_vals(f["ac"][c])) for c in range(nc)]
    q = [[int(v) for v in quant[c]] for c in range(nc)]
    return JW.write(planes, q, sampling, tables, f["width"], f["height"], dqt16=any(v > 255 for t in q for v in t))


@functools.lru_cache(maxsize=None)
def synthetic_set():
    """Every synthetic family of jpeg_cases as it is, and -- where it has a restart interval and its point survives (the symbols, the
    FF bytes, the layout; not the restart markers or the content of the MCU padding) -- again as a single long run."""
    out = {}
    for name, s in JC.synthetic().items():
        out[name] = s.data
        if JR.parse(s.data)["restart"] and name not in ("sweep_dri1", "sweep_dri4"):       # sweep_dri0 is that file already
            out[name + "_one_run"] = repack(s.data)
    return out


def gray_run_of(nbytes, seed, side=5):
    """A gray (side, side) file, (5, 5) unless given, behind the standard luma tables whose single run is exactly nbytes long: ten sparse random blocks, then
    coefficients added to the other fifteen -- 255s (18 bits each) up to some 40 bytes short, then +-1 (three bits each: run 0,
    size 1) until the length is met."""
    luma = JC.standard_tables()[0]
    plane = JC.pool_planes(np.random.default_rng(seed), [(side, side)], sizes=8, runs=9, most=12)[0]
    plane[2:, :, 1:] = 0
    slots = [(by, bx, k) for by in range(2, side) for bx in range(side) for k in range(1, 60)]

    def build(nbig, nsmall):
        assert nbig + nsmall <= len(slots)
        p = plane.copy()
        for j, (by, bx, k) in enumerate(slots[:nbig + nsmall]):
            p[by, bx, JR.ZIGZAG[k]] = (255 if j < nbig else 1) * (1 if k % 2 else -1)
        data = JW.write([p], [JC.QUANT_Y], [(1, 1)], [luma], 8 * side, 8 * side)
        return data, len(JR.parse(data)["runs"][0])

    nbig = nsmall = 0
    data, have = build(0, 0)
    while nbytes - have > 40:
        nbig += max(1, (nbytes - have - 40) * 8 // 20)
        data, have = build(nbig, 0)
    while have != nbytes:
        assert have < nbytes, "the base file is already longer"
        nsmall += max(1, ((nbytes - have) * 8 - 8) // 3)
        data, have = build(nbig, nsmall)
    return data


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> (bytes, what it is for)."""
    rng = np.random.default_rng(700)
    luma, out = JC.standard_tables()[0], {}
    # 1024 bytes = 32 segments of 256 bits = 8 of 1024: the last segment ends with the run, holds one byte more, is one byte short
    for n in (1024, 1025, 1023):
        out[f"run_{n}_bytes"] = gray_run_of(n, 11)
    # 15 and 16 segments of 256 bits: just below the default threshold (not split: path 0 there) and just at it
    out["run_480_bytes"] = gray_run_of(480, 12)
    out["run_481_bytes"] = gray_run_of(481, 12)
    # 63 coefficients of size 9 or 10 per block: about 1600 bits, six segments of 256 bits and more than one of 1024, so most
    # segments own no block
    dense = np.zeros((3, 3, 64), np.int64)
    dense[..., 1:] = rng.integers(256, 1024, (3, 3, 63)) * rng.choice([-1, 1], (3, 3, 63))
    dense[..., 0] = rng.integers(-500, 500, (3, 3))
    out["dense_blocks"] = JW.write([dense], [JC.QUANT_Y], [(1, 1)], [luma], 24, 24)
    # DC differences of category 11 with alternating signs in scan order, another pair of values per component, so that the three
    # scanned predictors differ and each segment's sums are large
    planes = JC.pool_planes(rng, JW.padded_grids(64, 64, JC.S420), sizes=8, runs=6, most=8)
    for c, (lo, hi) in enumerate([(-1024, 1023), (-1000, 1047), (-600, 1400)]):
        for j, (by, bx) in enumerate(JC.scan_blocks(64, 64, JC.S420, c)):
            planes[c][by, bx, 0] = (lo, hi)[(j + c // 2) % 2]
    out["dc_category_11"] = JW.write(planes, [JC.QUANT_Y, JC.QUANT_CB, JC.QUANT_CR], JC.S420, JC.std3(), 64, 64)
    # restart interval 8 of 16 MCUs: two runs in one image, each split
    planes = JC.pool_planes(rng, JW.padded_grids(64, 64, JC.S420), sizes=8, runs=6, most=9)
    out["two_long_runs"] = JW.write(planes, [JC.QUANT_Y, JC.QUANT_CB, JC.QUANT_CR], JC.S420, JC.std3(), 64, 64, restart=8)
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Grid (8, 8): two marker-less 4:2:0 files, two with a marker per MCU row (4 runs each), a gray one, the two-run file, and a
    file with one scan per component, which the device refuses."""
    files = [JC.encode(JC.noisy(64, 64, 21), quality=92), JC.encode(JC.noisy(64, 64, 22), quality=85, restart_marker_rows=1),
             JC.encode(JC.noisy(64, 64, 23, gray=True), quality=95), JC.three_scans().data, JC.encode(smooth(64, 64, 4), quality=97),
             JC.encode(JC.noisy(64, 64, 24), quality=95, restart_marker_rows=1), crafted()["two_long_runs"]]
    return files, 3


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pillow_set()))
def test_pillow_files_converge_for_certain(name, setting):
    data = pillow_set()[name]
    _, path = split_and_compare([data], grid_of(data), setting, None, name, certain=True)
    assert path == [1], (name, path)                              # the scan is long enough to be split in both settings


@pytest.mark.parametrize("name", sorted(synthetic_set()))
def test_synthetic_families(name, setting):
    """rounds 64, the most the call takes: the long files (8 KB: 256 segments of 256 bits) need not converge, and `path` must say
    what the restatement says."""
    data = synthetic_set()[name]
    split_and_compare([data], grid_of(data), setting, 64, name)


@pytest.mark.parametrize("name", sorted(crafted()))
def test_crafted_runs(name, setting):
    data = crafted()[name]
    plan, path = split_and_compare([data], grid_of(data), setting, None, name, certain=True)
    sb, _ = setting
    if name == "run_480_bytes":
        assert path == [0 if sb == 256 else 1]                    # 15 segments of 256 bits: below the threshold of 16
    else:
        assert path == [1], (name, path)
    if name == "two_long_runs":
        assert plan.nruns == 2


def test_mixed_batch_with_a_refused_file(setting):
    files, refused = mixed_batch()
    sb, min_seg = setting
    plan = dm.prepare_jpeg_batch(files, grid=(8, 8))
    assert plan.nbad == 1 and plan.status[refused] < 0
    _, longest, _ = SR.predict(plan, sb, 0, min_seg)
    rounds = longest - 1
    assert rounds <= 64
    want, _, _ = SR.predict(plan, sb, rounds, min_seg)
    assert want[refused] == 0 and set(want) <= {0, 1} and want.count(1) >= 4, want
    a, b = Outputs(len(files), (8, 8)), Outputs(len(files), (8, 8))
    dm.decode_jpeg_batch(plan, "cuda", out=a.t)
    run_split(plan, b, sb, rounds)
    a.check("mixed plain", written=False, path=False)
    b.check("mixed split", written=False)
    assert b.path.tolist() == want
    assert b.t[3].tolist() == plan.status[:len(files)].tolist() and b.t[3][refused] < 0      # the host's refusal is kept
    for x, y in zip(a.t, b.t):
        assert torch.equal(x, y)
    for i, data in enumerate(files):
        if i == refused:                                          # not a single element of its slots was written
            assert bool((b.t[0][i] == b.g[0].canary).all()) and bool((b.t[1][i] == b.g[1].canary).all())
            continue
        for got, ref in zip(b.t, host(data)):
            assert torch.equal(got[i].cpu(), ref), i


@pytest.mark.parametrize("rounds", [0, 1, 2])
def test_few_rounds_fall_back_exactly_where_the_restatement_says(rounds, setting):
    """The same bits whatever `rounds`; with none, every run of more than one segment whose guessed entries are not all true fails
    verify and is decoded by the one-lane walk."""
    files = [f for i, f in enumerate(mixed_batch()[0]) if i != mixed_batch()[1]]
    _, path = split_and_compare(files, (8, 8), setting, rounds, f"rounds {rounds}")
    if rounds == 0:
        assert all(p in (0, 2) for p in path), path               # 0: the file with a marker per MCU row, where its runs are too short
    assert 2 in path


@pytest.fixture
def small_grids():
    """Two workgroups per launch and five lanes per wave: every grid-stride loop of the split launches goes round again."""
    L.set_option("jpeg_split_wgs", 2)
    L.set_option("jpeg_lanes", 5)
    yield
    L.set_option("jpeg_split_wgs", 0)
    L.set_option("jpeg_lanes", 0)


def test_every_grid_stride_loop_goes_round_again(small_grids, setting):
    files = [f for i, f in enumerate(mixed_batch()[0]) if i != mixed_batch()[1]]
    plan, path = split_and_compare(files, (8, 8), setting, None, "two workgroups", certain=True)
    # more runs than workgroups, more slots than 2 x 5 lanes
    assert plan.nruns > 2 and plan.stream_bytes * 8 // setting[0] > 2 * 5
    assert path.count(1) >= 4


@pytest.fixture
def full_waves():
    L.set_option("jpeg_min_seg", 2)
    L.set_option("jpeg_lanes", 64)
    yield 256, 2
    L.set_option("jpeg_min_seg", 0)
    L.set_option("jpeg_lanes", 0)


def test_segments_behind_two_table_sets_share_a_wave(full_waves):
    """A file behind the standard tables and one behind long tables of its own, 38 and 20 segments of 256 bits in the 64 lanes of one
    wave: no table set serves the whole wave, so every pass, the write pass included, reads the tables from global memory (a wave of
    one file, as in the tests above, stages them)."""
    files = [JC.standard_420(7, 96, 64, restart=0).data, JC.long_codes().data]
    plan, path = split_and_compare(files, (8, 12), full_waves, None, "two table sets", certain=True)
    offset, nbytes = (int(v) for v in plan.runs[1, :2])
    assert path == [1, 1] and plan.ntables > 4 and offset * 8 // 256 + 1 + -(-nbytes * 8 // 256) <= 64     # the second run's last slot


def test_graph_capture_and_replay_with_other_files(setting):
    """One capture; the plan's device buffers are refilled from a second set of files of the same sizes -- the colour files in another
    order, the gray files with other content in runs of the same lengths: as many runs and tables, and no more stream bytes than
    the captured plan (a file's region depends on how many FF bytes it stuffs) -- and the replay equals the eager result for that set."""
    sb, min_seg = setting
    colour = [f for i, f in enumerate(mixed_batch()[0]) if i != mixed_batch()[1]]
    sets = [colour + [gray_run_of(1024, 51, 8), gray_run_of(700, 52, 8)], colour[::-1] + [gray_run_of(1024, 53, 8), gray_run_of(700, 54, 8)]]
    plans = sorted((dm.prepare_jpeg_batch(f, grid=(8, 8)) for f in sets), key=lambda p: -p.stream_bytes)
    first, second = plans                                         # the captured plan is the one with more stream bytes
    files = sets[0]
    assert first.nbad == second.nbad == 0
    assert (first.nruns, first.ntables, first.n) == (second.nruns, second.ntables, second.n) and second.stream_bytes <= first.stream_bytes
    rounds = max(SR.predict(p, sb, 0, min_seg)[1] for p in plans) - 1
    assert rounds <= 64
    eager = []
    for plan in (first, second):
        o = Outputs(len(files), (8, 8))
        run_split(plan, o, sb, rounds)
        o.check("eager")
        eager.append([t.clone() for t in o.t] + [o.path.clone()])
    assert not torch.equal(eager[0][0], eager[1][0])
    dev = [t.clone() for t in dm.upload_jpeg_plan(first, "cuda")]
    out = Outputs(len(files), (8, 8))
    scratch = dm.jpeg_split_scratch(first, sb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # warm-up outside the capture, as torch asks
        dm.launch_jpeg_decode(first, dev, out.t, split=True, seg_bits=sb, rounds=rounds, path=out.path, scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dm.launch_jpeg_decode(first, dev, out.t, split=True, seg_bits=sb, rounds=rounds, path=out.path, scratch=scratch)
    for plan, want in ((second, eager[1]), (first, eager[0]), (second, eager[1])):
        for d, h in zip(dev, plan.buffers()):
            d[:h.shape[0]].copy_(h)                                # the stream may be shorter than the captured plan's
        out.t[2].copy_(dev[4])
        out.t[3].copy_(dev[5])
        out.t[0].fill_(out.g[0].canary)
        out.t[1].fill_(out.g[1].canary)
        graph.replay()
        out.check("replay")
        for got, ref in zip(list(out.t) + [out.path], want):
            assert torch.equal(got, ref)


def test_convenience_call_and_defaults():
    """decode_jpeg_batch(split=True) with the default seg_bits and rounds, and read_coefficients_batch_device(split=True)."""
    data = JC.encode(JC.noisy(128, 128, 21), quality=95)            # 16 segments of the default size and more: split
    plan = dm.prepare_jpeg_batch([data, data], grid=(16, 16))
    Y, C, Q, st, path = dm.decode_jpeg_batch(plan, "cuda", split=True, return_path=True)
    assert len(dm.decode_jpeg_batch(plan, "cuda")) == 4 and len(dm.decode_jpeg_batch(plan, "cuda", split=True)) == 4
    want, _, _ = SR.predict(plan, dm.JPEG_SPLIT_SEG_BITS, dm.JPEG_SPLIT_ROUNDS)
    assert path.tolist() == want and want == [1, 1] and st.tolist() == [0, 0]
    Y2, C2, Q2 = dm.read_coefficients_batch_device([data, data], grid=(16, 16), device="cuda", split=True)
    for i in range(2):
        for got, got2, ref in zip((Y, C, Q), (Y2, C2, Q2), host(data)):
            assert torch.equal(got[i].cpu(), ref) and torch.equal(got2[i].cpu(), ref)


def test_loader_with_jpeg_split_yields_the_host_tensors(tmp_path):
    from rgb_no_more_amd.loader import DCTBatchLoader
    paths = []
    for i in range(12):
        p = tmp_path / f"s{i}.jpg"
        kw = {"restart_marker_rows": 1} if i % 4 == 3 else {}
        p.write_bytes(JC.encode(JC.noisy(128, 128, 60 + i, gray=(i == 5)), quality=95, **kw))
        paths.append(str(p))
    labels = list(range(12))
    kw = dict(batch_size=5, device="cuda", grid=(16, 16), shuffle=False)
    a = [(Y.clone(), C.clone(), Q.clone(), lab.clone()) for (Y, C, Q), lab in DCTBatchLoader(paths, labels, decode="host", **kw)]
    b = [(Y.clone(), C.clone(), Q.clone(), lab.clone()) for (Y, C, Q), lab in DCTBatchLoader(paths, labels, decode="device", jpeg_split=True, **kw)]
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)
    # the files are long enough for the default segment size to split them
    plan = dm.prepare_jpeg_batch(paths[:3], grid=(16, 16))
    assert all(SR.predict(plan, dm.JPEG_SPLIT_SEG_BITS, 0)[0]), "a file of the folder is too short to be split"
