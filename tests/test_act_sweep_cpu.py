"""CPU side of the activation sweeps (tests/act_sweep_ref.py; the device side is tests/test_act_sweep.py).

1. Coverage: the layouts put every value of a set at both column parities and, on the GEMM shapes, into two row tiles; the
   block-level slices cover the set.
2. Bounds and predictions: an fp32 emulation of common.h gelu_pair_fast (exact reciprocal and exp2) and torch.tanh in fp32 pass
   assertions 4 to 6 for all of S_bf16, S_f16 and S_f32 (worst ratios printed, -s), and a Python restatement of gelu_table.h
   gelu_table_pairs4's key arithmetic, run on a table built from the emulation, reproduces that table for every input.
3. Seeded defects: each fails at least one assertion (the last one is the defect the device sweep found and fixed).
"""
import math

import numpy as np
import pytest
import torch

import act_sweep_ref as S
from act_sweep_ref import BF16, F16, F32

# (M, N, K, rows of an output tile, passes) of tests/test_act_sweep.py's GEMM paths
GEMM_SHAPES = [(256, 256, 256, 128, 2),        # gemm_nt_kernel
               (256, 256, 256, 32, 2),         # gemm_nt_small_kernel
               (4096, 384, 192, 128, 2),       # gemm_nt_wres_kernel (any tile height below M - K works: rows repeat every K)
               (8193, 384, 256, 224, 2),       # kp7
               (16384, 768, 256, 256, 1)]      # kp8: one pass


@pytest.fixture(scope="module")
def emu():
    out = {}
    for dt in (BF16, F16):
        u = S.all_patterns(dt).float().numpy()
        g32, d32 = S.emu_gelu_pair(u)
        out[dt] = S.emu_tables(dt, g32, d32)
    out["full"] = S.emu_full()
    out["win"] = S.scan_window(out["full"])
    return out


# ------------------------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("M,N,K,tile,passes", GEMM_SHAPES)
def test_gemm_layout_covers_both_parities_and_two_row_tiles(M, N, K, tile, passes):
    nvals = 65536
    cols, lo, hi = [], None, None
    for p in range(passes):
        k, n = S.gemm_slots(nvals, N, K, p)
        assert torch.unique(k * N + n).numel() == nvals                    # no two values share a slot
        assert int(k.max()) < K and int(n.max()) < N
        cols.append(n)
        first, last = k // tile, (k + ((M - 1 - k) // K) * K) // tile      # tiles of the first / last row m = k (mod K)
        lo = first if lo is None else torch.minimum(lo, first)
        hi = last if hi is None else torch.maximum(hi, last)
    assert bool((hi > lo).all())
    if passes == 2:
        assert bool(((cols[0] + cols[1]) % 2 == 1).all())
    # the operands deliver W[n, m % K] and nothing else
    vals = torch.arange(1, 1 + 4096, dtype=torch.float64)
    A, W, k, n = S.gemm_operands(vals, 2 * K + 1, N, K, passes - 1)
    u = A @ W.T
    assert torch.equal(u[k, n], vals) and torch.equal(u[k + K, n], vals) and int((A != 0).sum()) == 2 * K + 1
    assert torch.equal(u, u[torch.arange(2 * K + 1) % K])


def test_non_finite_values_never_sit_in_w():
    vals = S.all_patterns(BF16)
    A, W, k, n = S.gemm_operands(vals, 256, 256, 256, 0)
    assert bool(torch.isfinite(W).all()) and bool(torch.isfinite(A @ W.T.float().to(A.dtype)).all())
    b = S.to_bits(W[n, k])
    fin = S.is_finite_bits(torch.arange(65536, dtype=torch.int32), BF16)
    assert torch.equal(b[fin], torch.arange(65536, dtype=torch.int32)[fin]) and bool((b[~fin] == 0).all())


@pytest.mark.parametrize("n", [3, 254, 256, 2046, 2048, 12240])
def test_bias_layout_covers_both_parities(n):
    v = torch.arange(1, n + 1, dtype=F32)
    off, need = S.bias_slots(n)
    b, off2 = S.bias_vector(v, -(-need // 384) * 384)
    assert off == off2 and off % 2 == 1
    assert torch.equal(b[:n], v) and torch.equal(b[off:off + n], v) and float(b.sum()) == 2 * float(v.double().sum())


def test_block_slices_cover_the_set_at_both_parities():
    blk0, col0, nblk = S.block_slots(65536, 0)
    blk1, col1, nblk1 = S.block_slots(65536, 1)
    assert nblk == nblk1 == 86 and nblk <= 8 * 12                           # eight launches of depth 12
    for blk, col in ((blk0, col0), (blk1, col1)):
        assert torch.unique(blk * S.HID + col).numel() == 65536 and int(blk.max()) < nblk
    assert bool(((col0 + col1) % 2 == 1).all())


def test_edge_slice_holds_every_window_edge_at_both_parities(emu):
    A0, P1, N1, _ = emu["win"]
    sl = S.edge_slice(A0, P1, N1)
    assert sl.shape == (S.HID,)
    fin = S.is_finite_bits(torch.from_numpy(sl).to(torch.int32), BF16)
    assert bool(fin.all())
    for name, v in S.window_edges(A0, P1, N1).items():
        at = np.nonzero(sl == v)[0]
        assert {int(c) % 2 for c in at} == {0, 1}, (name, at)


def test_input_sets():
    v = S.s_f32()
    assert bool(torch.isfinite(v).all()) and bool((v[1:].double() >= v[:-1].double()).all())
    assert torch.unique(S.bits32(v)).numel() == v.numel()
    for dt in (BF16, F16):
        p = S.all_patterns(dt)
        fin = torch.isfinite(p)
        assert int(fin.sum()) == {BF16: 65280, F16: 63488}[dt]
        assert bool(torch.isin(S.bits32(p[fin].float()), S.bits32(v)).all())
        assert torch.equal(S.to_bits(p), torch.arange(65536, dtype=torch.int32))
    assert 65280 < v.numel() <= 65280 + 63488


@pytest.mark.parametrize("dt", [BF16, F16])
def test_tie_inputs_round_as_stated(dt):
    u, want = S.s_tie(dt)
    assert u.numel() % 6 == 0 and u.numel() > 11000
    assert torch.equal(S.to_bits(u.to(dt)), want)                           # torch rounds to nearest even
    # the three of a group are distinct fp32 values one ulp apart, and the outer two round apart
    g = S.bits32(u).view(2, -1, 3)
    assert bool((g[..., 1] - g[..., 0] == 1).all()) and bool((g[..., 2] - g[..., 1] == 1).all())
    w = want.view(2, -1, 3)
    assert bool((w[..., 0] == w[..., 1]).all()) and bool((w[..., 2] == w[..., 1] + 1).all())


# --------------------------------------------------------------------------------------------------- bounds and predictions
def test_reference_and_hardware_term():
    x = torch.linspace(-3, 30, 20001, dtype=torch.float64)
    erf_form = 0.5 * x * (1.0 + torch.special.erf(x * S.SQRT1_2))            # tests/test_kernel_edges.py gelu64
    assert float(((S.gelu64(x) - erf_form).abs() / erf_form.abs().clamp_min(1e-300)).max()) < 1e-12
    derf = 0.5 * (1.0 + torch.special.erf(x * S.SQRT1_2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    assert float((S.dgelu64(x) - derf).abs().max()) < 1e-15
    # the left tail keeps its relative precision: gelu(-12) = -12 Phi(-12) = -2.13e-32
    assert abs(float(S.gelu64(torch.tensor(-12.0, dtype=torch.float64))) / -2.1312e-32 - 1) < 1e-3
    t = torch.linspace(1e-6, 1.0, 100001, dtype=torch.float64)
    a = S.AS_A
    P = sum(a[i] * t ** (i + 1) for i in range(5))
    dP = sum((i + 1) * a[i] * t ** (i + 1) for i in range(5))                # t P'(t)
    L = dP / P
    assert 3.4 < float(L.max()) <= S.HW_L and float(L.min()) >= 0.9


@pytest.mark.parametrize("dt", [BF16, F16])
def test_emulation_meets_assertions_2_to_6(emu, dt):
    g, d = emu[dt]
    where = f"emulation {S.NAMES[dt]}"
    w = S.check_gelu_tables(where, dt, g, d, emu["full"], emu["win"][:3], exact=(dt == BF16))
    S.assert_nonfinite(where, dt, g)
    print(f"\n[{where}] worst bound ratios {w}; non-finite {S.nonfinite_summary(dt, g, d)}")
    h = S.to_bits(torch.tanh(S.all_patterns(dt).float()).to(dt))
    print(f"[{where}] tanh {S.check_tanh_table(where, dt, h)}")


def test_emulation_meets_the_bound_in_fp32():
    u = S.s_f32()
    g, d = (torch.from_numpy(t) for t in S.emu_gelu_pair(u.numpy()))
    w = (S.assert_bound("emulation f32", "gelu", u, g, F32), S.assert_bound("emulation f32", "dgelu", u, d, F32))
    S.assert_gelu_properties("emulation f32", u, g)
    h = torch.tanh(u)
    wt = S.assert_bound("emulation f32", "tanh", u, h, F32)
    neg_of = torch.searchsorted(_order_key(u), _order_key(-u))             # u is ascending: index of -u
    S.assert_tanh_properties("emulation f32", u, h, neg_of)
    print(f"\n[emulation f32] worst bound ratios gelu {w[0]:.4f} gelu' {w[1]:.4f} tanh {wt:.4f}")


def _order_key(v):
    k = S.bits32(v).to(torch.int64)
    return torch.where(k < 0, -(k & 0x7FFFFFFF) - 1, k)


def test_key_arithmetic_reproduces_the_table_for_every_input(emu):
    full = emu["full"]
    A0, P1, N1, gpn = emu["win"]
    assert 0x100 <= A0 < P1 <= N1 < 0x7F80
    img = S.build_image(full, A0, P1, N1, gpn)
    assert 4 * len(img) <= 13328                                            # gelu_table.h GELU_TAB_BYTES
    b = np.arange(65536)
    g, d = S.table_lookup(b, img, A0, P1, N1)
    g, d = torch.from_numpy(g).to(torch.int32), torch.from_numpy(d).to(torch.int32)
    assert S.assert_full_bits("table lookup", g, d, full, (A0, P1, N1)) == 0
    S.assert_below_window("table lookup", g, d)
    # non-finite inputs: +inf and NaNs of the positive sign pass through (gelu = u), -inf is clamped like every large negative input
    # (-0, gelu' = 0; the arithmetic gives NaN there: recorded in DESIGN.md), NaNs of the negative sign stay NaNs
    S.assert_nonfinite("table lookup", BF16, g)
    assert int(g[0x7F80]) == 0x7F80 and int(g[0x7FC0]) == 0x7FC0 and int(g[0xFF80]) == 0x8000 and int(g[0xFFC0]) == 0xFFC0


# ----------------------------------------------------------------------------------------------------------- seeded defects
def _lookup_tables(emu, **kw):
    A0, P1, N1, gpn = emu["win"]
    img = kw.pop("img", None)
    img = S.build_image(emu["full"], A0, P1, N1, gpn) if img is None else img
    g, d = S.table_lookup(np.arange(65536), img, A0, P1, N1, **kw)
    return torch.from_numpy(g).to(torch.int32), torch.from_numpy(d).to(torch.int32)


def _check(emu, g, d, dt=BF16):
    return S.check_gelu_tables("seeded", dt, g, d, emu["full"], emu["win"][:3], exact=(dt == BF16))


def test_sound_tables_pass(emu):
    _check(emu, *_lookup_tables(emu))
    _check(emu, *emu[BF16])
    _check(emu, *emu[F16], dt=F16)


def test_defect_one_table_entry_off_by_one_ulp(emu):
    A0, P1, N1, gpn = emu["win"]
    for idx, delta in ((5, 1), (P1 - A0 + 7, 1 << 16)):                       # a gelu difference D, a gelu' entry
        img = S.build_image(emu["full"], A0, P1, N1, gpn)
        img[idx] += delta
        with pytest.raises(AssertionError, match="differ from full65536"):
            _check(emu, *_lookup_tables(emu, img=img))


@pytest.mark.parametrize("kw", [dict(dklo=-1), dict(dkpos=1), dict(dkneg=1)], ids=["A0", "P1", "N1"])
def test_defect_key_off_by_one_at_a_window_edge(emu, kw):
    """One clamp constant of the packed key arithmetic off by one, in the direction that leaves its entry (the window is found
    per exponent row, so the other direction can be harmless: the entry next to an edge may already equal the closed form)."""
    with pytest.raises(AssertionError, match="differ from full65536"):
        _check(emu, *_lookup_tables(emu, **kw))


def test_defect_halves_of_a_pair_swapped(emu):
    g, d = emu[BF16]
    swap = torch.arange(65536) ^ 1                                            # value j sits next to value j ^ 1 in pass 0
    with pytest.raises(AssertionError):
        _check(emu, g[swap], d[swap])
    # at ONE boundary only: the pair that straddles nothing but holds P1 - 1 | P1 - 2
    P1 = emu["win"][1]
    g2, d2 = g.clone(), d.clone()
    pair = torch.tensor([P1 - 2, P1 - 1])
    g2[pair], d2[pair] = g[pair.flip(0)], d[pair.flip(0)]
    with pytest.raises(AssertionError, match="P1-1"):
        _check(emu, g2, d2)


def test_defect_negative_nan_clamped_to_minus_zero(emu):
    """The lookup as the sweep found it: the 127 NaN patterns with the sign bit set give gelu = -0."""
    with pytest.raises(AssertionError, match="127 NaN inputs"):
        _check(emu, *_lookup_tables(emu, nan_fix=False))


def test_defect_sign_dropped_beyond_n1(emu):
    with pytest.raises(AssertionError):
        _check(emu, *_lookup_tables(emu, drop_sign_beyond_n1=True))
    g, d = _lookup_tables(emu, drop_sign_beyond_n1=True)
    with pytest.raises(AssertionError, match="sign"):                         # also without the bit comparison
        S.assert_gelu_properties("seeded", S.all_patterns(BF16), S.from_bits(g, BF16))


def _tie_results(dt, rounding):
    u, want = S.s_tie(dt)
    if rounding == "rne":
        ur = u.to(dt).float()
    elif rounding == "trunc":
        assert dt == BF16
        ur = (S.bits32(u) & -65536).view(F32)
    else:
        ur = u
    g32, d32 = S.emu_gelu_pair(ur.numpy())
    return want, S.emu_tables(dt, g32, d32)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_ties_pass_with_rounding_to_nearest_even(emu, dt):
    want, (g, d) = _tie_results(dt, "rne")
    S.assert_ties("ties", dt, want, g, emu[dt][0])
    S.assert_ties("ties", dt, want, d, emu[dt][1])


@pytest.mark.parametrize("rounding", ["trunc", "none"])
def test_defect_pre_activation_not_rounded_to_nearest(emu, rounding):
    want, (g, d) = _tie_results(BF16, rounding)
    with pytest.raises(AssertionError, match="tie inputs"):
        S.assert_ties("ties", BF16, want, g, emu[BF16][0])


def test_defect_fp16_subnormal_results_flushed(emu):
    g, d = emu[F16]
    flushed = torch.where(S.is_subnormal_bits(g, F16), g & 0x8000, g)
    assert int((flushed != g).sum()) > 1000
    with pytest.raises(AssertionError, match="beyond the fp64 bound"):
        _check(emu, flushed, d, dt=F16)


@pytest.mark.parametrize("dt", [BF16, F16])
def test_defect_derivative_of_the_neighbouring_input(emu, dt):
    g, d = emu[dt]
    nb = torch.arange(65536)
    nb = torch.where((nb & 0x7FFF) < 0x7BFF, nb + 1, nb)
    with pytest.raises(AssertionError):
        _check(emu, g, d[nb], dt=dt)
