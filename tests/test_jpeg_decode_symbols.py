"""The device JPEG entropy decode (csrc/jpeg_decode.hip, jpeg_walk.h) on hand-written streams: the synthetic files of
tests/jpeg_cases.py, whose symbols, tables, stuffed bytes, layouts and run counts are chosen (tests/test_jpeg_writer_cpu.py asserts
what each holds).  Bit for bit against the coefficients the files were written from AND against the host libjpeg reader, into the
guarded outputs of tests/test_jpeg_decode_kernels.py: every status 0, every element written, nothing outside.  Well-formed files
only: damaged streams stay on the CPU (tools/jpeg_scan_check.cpp)."""
import time

import pytest
import torch

import jpeg_cases as JC
from rgb_no_more_amd import lib as L
from test_jpeg_decode_kernels import decode_and_compare

pytestmark = pytest.mark.gpu

MAX_WGS = 4096                   # jpeg_decode.hip: workgroups of the launch at most; beyond it the grid-stride loop takes more trips


@pytest.fixture
def lanes(request):
    L.set_option("jpeg_lanes", request.param)
    yield request.param
    L.set_option("jpeg_lanes", 0)


def decode_and_compare_with_source(cases, grid, where):
    """decode_and_compare (host reader, guards, status) and the writer's source coefficients."""
    t0 = time.perf_counter()
    plan, out = decode_and_compare([s.data for s in cases], grid, where)
    Y, C, Q, _ = out.t
    Y, C, Q = Y.cpu(), C.cpu(), Q.cpu()
    for i, s in enumerate(cases):
        hb, wb = s.grid
        assert torch.equal(Y[i].reshape(hb, wb, 64), torch.from_numpy(s.Y)), (where, s.name, "Y")
        want = torch.zeros_like(C[i]) if s.C is None else torch.from_numpy(s.C).reshape(C[i].shape)
        assert torch.equal(C[i], want), (where, s.name, "CbCr")
        assert torch.equal(Q[i, :len(s.quant)].reshape(-1, 64), torch.from_numpy(s.quant)), (where, s.name, "quant")
    print(f"{where}: {len(cases)} files, {plan.nruns} runs, {time.perf_counter() - t0:.2f} s")
    return plan


@pytest.mark.parametrize("lanes", [64, 0, 5], indirect=True)
def test_sweep_of_every_symbol(lanes):
    """All 162 symbols of both standard AC tables, every size at both ends in both signs, DC categories 0..11, ZRL chains, blocks
    without EOB, as one run, as 42 and as 11: 54 runs, which 5 per wave split inside the files."""
    plan = decode_and_compare_with_source(JC.sweep(), (11, 13), f"sweep, {lanes} runs per wave")
    assert plan.nruns == 1 + 42 + 11 and plan.ntables == 4


@pytest.mark.parametrize("lanes", [64, 0, 5], indirect=True)
def test_long_codes_alone_stage_six_distinct_tables(lanes):
    """One run, so the wave's table set is this file's: six distinct tables in the six LDS slots.  Cb and Cr differ in tables and
    content: a slot or a select that takes one for the other cannot give these bits."""
    s = JC.long_codes()
    plan = decode_and_compare_with_source([s], (8, 12), f"long codes alone, {lanes} runs per wave")
    assert plan.nruns == 1 and plan.ntables == 6 and len(set(plan.images[0, 5:11].tolist())) == 6


@pytest.mark.parametrize("lanes", [64, 0, 5], indirect=True)
def test_long_codes_beside_a_standard_file_read_global_tables(lanes):
    """With 64 or 5 runs per wave the file shares its wave with a standard-table file's runs: no common table set, the lanes read
    the batch's table array.  The long-code file comes second, so its tables are not the first of the array either."""
    cases = [JC.standard_420(7, 96, 64, restart=7), JC.long_codes()]
    plan = decode_and_compare_with_source(cases, (8, 12), f"long codes in a mixed wave, {lanes} runs per wave")
    assert plan.nruns == 5 and plan.ntables == 10 and min(plan.images[1, 5:11].tolist()) >= 4


@pytest.mark.parametrize("lanes", [64, 0, 5], indirect=True)
def test_stuffed_bytes_and_fill_bytes(lanes):
    """Data bytes FF are frequent; runs end in FF in front of RSTn and EOI, behind 0 and 2 fill bytes; run lengths of every residue
    mod 4, down to one byte."""
    plan = decode_and_compare_with_source(JC.stuffing(), (5, 7), f"stuffing, {lanes} runs per wave")
    assert plan.nruns == 35 + 35 + 12


@pytest.mark.parametrize("name", ["444_grid_1x1", "422_grid_1x5", "440_grid_5x1", "gray_0x22", "gray_0x11", "gray_0x41", "420_ids",
                                  "420_padding"])
def test_layouts_each_as_its_own_batch(name):
    """Sampling layouts other than 4:2:0 (3 and 4 blocks per MCU), one-component frames whose sampling byte is not 0x11, component
    ids other than 1, 2, 3, padding blocks full of large coefficients on both edges."""
    s = JC.layouts()[name]
    decode_and_compare_with_source([s], tuple(s.grid), name)


@pytest.mark.parametrize("lanes", [1, 2, 0], indirect=True)
def test_many_runs_take_the_grid_stride_loop_round_again(lanes):
    """8275 runs of 241 small files.  One run per wave: 8275 waves' worth of work on 4096 workgroups, three trips for the first 83.
    Two: 4138 pairs, a second trip for 42 workgroups; a file has an odd number of runs and its neighbour other tables, so every
    other pair has no common table set: staging and global reads alternate within a workgroup's trips and between neighbours.
    0: the launch's own choice, 5 runs per wave, one trip.  A tile that a run left dirty, or tables staged over a reader, show as
    wrong coefficients: every block of every file is compared."""
    cases = JC.many_runs()
    plan = decode_and_compare_with_source(cases, (5, 7), f"many runs, {lanes} runs per wave")
    per = lanes or -(-plan.nruns // 2048)
    trips = -(-(-(-plan.nruns // per)) // MAX_WGS)
    print(f"many runs: {plan.nruns} runs, {per} per wave, {-(-plan.nruns // per)} waves' worth on {MAX_WGS} workgroups: {trips} trip(s)")
    if lanes:
        assert plan.nruns > MAX_WGS * lanes, "the second trip of the grid-stride loop was not reached"
        assert trips == (3 if lanes == 1 else 2)
    else:
        assert per == 5 and trips == 1
