"""The device JPEG entropy decode (csrc/jpeg_decode.hip, one lane per restart run) against the host libjpeg reader, bit for bit, into
guarded outputs (tests/kernel_check.py): every element written -- zeros included, without a fill launch -- and nothing outside.
Well-formed files only: damaged streams are exercised on the CPU (tools/jpeg_scan_check.cpp runs the same walk under sanitizers)."""
import functools

import pytest
import torch

import jpeg_cases as JC
import kernel_check as KC
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def host(data):
    """(Y [1, Hb, Wb, 8, 8], CbCr [2, Hbc, Wbc, 8, 8] (zeros for one component), quant [3, 8, 8] (unit chroma tables then))."""
    _, quant, Y, CbCr = dm.read_coefficients_bytes(data)
    hb, wb = Y.shape[1:3]
    if CbCr is None:
        CbCr = torch.zeros((2, (hb + 1) // 2, (wb + 1) // 2, 8, 8), dtype=torch.int16)
    q = torch.ones((3, 8, 8), dtype=torch.int16)
    q[:quant.shape[0]] = quant
    return Y, CbCr, q


class Outputs:
    """Guarded Y / CbCr / quant / status for n files of one grid."""

    def __init__(self, n, grid):
        hb, wb = grid
        hbc, wbc = (hb + 1) // 2, (wb + 1) // 2
        self.g = [KC.guarded(n * hb * wb, 64, torch.int16), KC.guarded(n * 2 * hbc * wbc, 64, torch.int16),
                  KC.guarded(n * 3, 64, torch.int16), KC.guarded(n, None, torch.int32)]
        self.t = (self.g[0].t.view(n, 1, hb, wb, 8, 8), self.g[1].t.view(n, 2, hbc, wbc, 8, 8), self.g[2].t.view(n, 3, 8, 8), self.g[3].t)

    def check(self, where):
        torch.cuda.synchronize()
        for g, name in zip(self.g, ("Y", "CbCr", "quant", "status")):
            g.check(f"{where} {name}")


def decode_and_compare(files, grid, where, out=None):
    plan = dm.prepare_jpeg_batch(files, grid=grid)
    assert plan.nbad == 0, plan.messages
    out = out or Outputs(len(files), grid)
    Y, C, Q, st = dm.decode_jpeg_batch(plan, "cuda", out=out.t)
    out.check(where)
    assert st.tolist() == [0] * len(files), st.tolist()
    for i, data in enumerate(files):
        Yh, Ch, Qh = host(data)
        assert torch.equal(Y[i].cpu(), Yh), (where, i, "Y")
        assert torch.equal(C[i].cpu(), Ch), (where, i, "CbCr")
        assert torch.equal(Q[i].cpu(), Qh), (where, i, "quant")
    return plan, out


@pytest.mark.parametrize("name", ["c64x64", "c48x80", "g40x56", "c37x53"])
def test_golden_files_one_by_one(name):
    """c37x53: partial MCUs on both edges (padding blocks decoded and dropped); g40x56: one component, unit chroma tables, zero chroma."""
    data = JC.g1_files()[name]
    hb, wb = host(data)[0].shape[1:3]
    decode_and_compare([data], (hb, wb), name)


@pytest.fixture
def lanes(request):
    """Runs per wave (option "jpeg_lanes"; 0: the launch's own choice, which is 1 for batches this small)."""
    L.set_option("jpeg_lanes", request.param)
    yield request.param
    L.set_option("jpeg_lanes", 0)


@pytest.mark.parametrize("lanes", [64, 0, 5], indirect=True)
def test_mixed_batch_of_more_than_one_wave(lanes):
    """82 runs (five files of 16, two of 1).  64 per wave: two waves, the second partly idle; the optimised file's tables differ
    from the others', so its wave reads the tables from global memory while the first stages the shared set in LDS.  5 per wave: 17
    waves, a launch of fewer than 64 lanes per wave with a ragged end."""
    files = JC.small_batch()
    plan, _ = decode_and_compare(files, (8, 8), f"mixed batch, {lanes} runs per wave")
    assert plan.nruns == 82 and plan.ntables > 4


@pytest.mark.parametrize("lanes", [64, 0], indirect=True)
def test_restart_intervals_and_gray_in_one_batch(lanes):
    p = JC.pillow_files()
    files = [p[k] for k in ("rst_blocks1", "rst_blocks2", "rst_blocks3", "rst_rows1", "gray_rst", "q30", "q100", "optimize")]
    decode_and_compare(files, (9, 13), f"restart batch, {lanes} runs per wave")


@functools.lru_cache(maxsize=None)
def full_size(restart_rows):
    kw = {"restart_marker_rows": 1} if restart_rows else {}
    return JC.encode(JC.noisy(512, 512, 30), quality=90, **kw)


@pytest.mark.parametrize("restart_rows", [0, 1])
def test_full_grid_file(restart_rows):
    """512 x 512 at quality 90: the real grid; one run of the whole scan, or 32 runs of one MCU row."""
    plan, _ = decode_and_compare([full_size(restart_rows)], (64, 64), f"512 x 512 restart_rows={restart_rows}")
    assert plan.nruns == (32 if restart_rows else 1)


def test_second_call_into_the_same_outputs_gives_the_same_bits():
    """The zero fill does not depend on what the outputs held: A, then B over it, then A again."""
    p = JC.pillow_files()
    A = [p["gray_rst"], p["q30"], p["rst_blocks2"]]
    B = [p["q100"], p["rst_rows1"], p["optimize"]]
    _, out = decode_and_compare(A, (9, 13), "first A")
    first = [t.clone() for t in out.t]
    decode_and_compare(B, (9, 13), "B over A", out=out)
    decode_and_compare(A, (9, 13), "A over B", out=out)
    for a, b in zip(first, out.t):
        assert torch.equal(a, b)


def test_convenience_call_and_refusal():
    p = JC.pillow_files()
    Y, C, Q = dm.read_coefficients_batch_device([p["q75"], p["gray_rst"]], grid=(9, 13), device="cuda")
    for i, k in enumerate(("q75", "gray_rst")):
        Yh, Ch, Qh = host(p[k])
        assert torch.equal(Y[i].cpu(), Yh) and torch.equal(C[i].cpu(), Ch) and torch.equal(Q[i].cpu(), Qh)
    with pytest.raises(dm.libjpeg_exception, match="bytes #1"):
        dm.read_coefficients_batch_device([p["q75"], JC.g1_files()["c64x64"]], grid=(9, 13), device="cuda")
