"""CPU side of tests/test_augment_edges.py (read tests/augment_ref.py's docstring first): the fp64 kernel-1 reference is anchored to
the oracle, the derived window admits a correct fp32 evaluation and its tie-share caps hold on the committed inputs, the work-split
restatement is checked against a brute-force count, the GPU file's case lists reach the regimes they claim on grids of 1024 and of
256 workgroups, every seeded defect of the numpy emulation is rejected by the same check functions the GPU file uses, and the oracle
agrees with the reference on flat images (tests/golden/g24_flat.npz, made by tests/golden/make_golden_flat.py)."""
import numpy as np
import pytest

import augment_ref as AR
import test_augment as TA
from oracle import dct_np as O
from rgb_no_more_amd import custom_transforms as CT

A16 = O.conversion_matrix(8, 2, np.float32)          # pinned to the reference's matrix by tests/golden/g3_convmat.npz
K = AR.weights()


def inputs(S):
    """The committed synthetic inputs of the resize cases: test_augment.synth, seed 2 (28-grid) / 8 (32-grid), 64 x 64 luma."""
    return TA.synth(2, 64, 64, seed=2 if S == 28 else 8)


def test_weights_are_the_sources_defaults():
    assert K == (9, 8, 12)


# ================================================================================================== anchor to the oracle
@pytest.mark.parametrize("S", [28, 32])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fp64_reference_rounds_to_the_oracle_and_the_oracle_passes_the_rule(S, mode):
    Y, Cc, quant = inputs(S)
    side = (2 * S, S, S // 2)[mode]
    for b in range(2):
        box = (2 * b, (64 - side) // 2 * 2 - 2 * b if side < 64 else 0, side, side) if side < 64 else (0, 0, 64, 64)
        flip = bool(b)
        m, planes = AR.k1_ref(Y[b], Cc[b], quant[b], box, S, A16)
        assert m == mode
        Yd, Cd = O.dequantize(Y[b], Cc[b], quant[b])
        i, j, h, w = box
        for nm, (raw, mag), T, Sp in (("Y", planes[0], O.crop(Yd, i, j, h, w), S), ("C", planes[1], O.crop(Cd, i // 2, j // 2, h // 2, w // 2), S // 2)):
            n32 = O.resize(T, Sp).astype(np.int64)                            # the fp32 oracle
            e = AR.window(raw, mag, mode)
            one = np.rint(raw - e) == np.rint(raw + e)
            assert np.array_equal(np.rint(raw)[one], n32[one]), (S, mode, nm)   # outside the tie window: the same integer
            got = AR.finish(n32, flip, True)
            worst, share = AR.check_k1(got, raw, mag, mode, flip, True, f"S{S} mode{mode} {nm}")      # asserts the cap
            print(f"S {S} mode {mode} {nm}: worst {worst:.4f}, two-valued share {100 * share:.4f} %, max e {e.max():.2e}")
            assert worst <= 1.0
            if mode == 1:
                assert share == 0.0 and np.array_equal(got, AR.finish(raw.astype(np.int64), flip, True))


def test_tie_share_of_the_issue_inputs():
    """seed 2, 64 x 64, luma, exactly this e: about 7.4 % for /2 (structural: the quarter-integers of the even/even frequencies) and
    below 0.01 % for x2."""
    Y, Cc, quant = TA.synth(4, 64, 64, seed=2)
    sh = {0: [], 2: []}
    for b in range(4):
        for side, mode in ((56, 0), (14, 2)):
            _, planes = AR.k1_ref(Y[b], Cc[b], quant[b], (2 * b, 8 - 2 * b, side, side), 28, A16)
            raw, mag = planes[0]
            e = AR.window(raw, mag, mode)
            sh[mode].append(float((np.rint(raw + e) > np.rint(raw - e)).mean()))
    print("two-valued shares, luma:", {m: [round(100 * v, 4) for v in s] for m, s in sh.items()})
    assert 0.06 < np.mean(sh[0]) <= 0.08 and max(sh[0]) <= AR.TIE_CAP[0]
    assert np.mean(sh[2]) < 1e-4 and max(sh[2]) <= AR.TIE_CAP[2]


# ================================================================================================== work split
def test_work_split_hands_every_item_to_exactly_one_wave():
    rng = np.random.default_rng(0)
    trials = [(1, 4), (1, 8192), (512, 4), (512, 8192), (7, 4096), (8, 1024)] + \
        [(int(rng.integers(1, 513)), int(rng.integers(4, 8193))) for _ in range(24)]
    for B, nwave in trials:
        S = (28, 32)[B & 1]
        modes = [int(v) for v in rng.integers(0, 3, B)]
        if B % 5 == 0:
            modes = [modes[0]] * B
        pfx = AR.cost_prefix(modes, S, K)
        waves = AR.work_split(pfx, nwave, modes, K)
        assert len(waves) == nwave
        count = [np.zeros(AR.items_of(m, S), np.int64) for m in modes]
        owner = [np.full(AR.items_of(m, S), -1, np.int64) for m in modes]
        for wave, visits in enumerate(waves):
            for b, j0, j1 in visits:
                n = AR.items_of(modes[b], S)
                assert j1 >= 1 and 0 <= j0 <= j1 <= n, (B, nwave, wave, b, j0, j1)
                assert 0 <= min(j0, j1 - 1) < n                                  # the fetch cursor starts on a valid item
                count[b][j0:j1] += 1
                owner[b][j0:j1] = wave
        # brute force: item j of image b starts at cost pfx[b] + j k and belongs to the wave whose share holds that start
        share, rem = divmod(pfx[-1], nwave)
        los = np.array([w * share + min(w, rem) for w in range(nwave + 1)])
        for b, m in enumerate(modes):
            assert (count[b] == 1).all(), (B, nwave, b, np.flatnonzero(count[b] != 1)[:4])
            starts = pfx[b] + np.arange(AR.items_of(m, S)) * K[m]
            assert np.array_equal(owner[b], np.searchsorted(los, starts, side="right") - 1), (B, nwave, b)


@pytest.mark.parametrize("wgs", [1024, 256])
@pytest.mark.parametrize("S", [28, 32])
def test_case_lists_reach_the_regimes_they_claim(S, wgs):
    nwave = 4 * wgs
    lens, empty = {0: set(), 1: set(), 2: set()}, False
    modes_alone = set()
    for _nm, sides in AR.small_cases(S):
        l, e = AR.regimes(sides, S, nwave, K)
        ms = {AR.mode_of(s, S) for s in sides}
        if len(ms) == 1:
            modes_alone |= ms
        for m in l:
            lens[m] |= l[m]
        empty |= e
    assert modes_alone == {0, 1, 2} and any(len({AR.mode_of(s, S) for s in sd}) == 3 for _n, sd in AR.small_cases(S))
    assert {0, 1, 2} <= lens[0] and {0, 1} <= lens[1] and empty          # the small batches: visits of 0, 1, 2 items and j0 == j1
    turns = set()
    for B in AR.TABLE_BATCHES:
        sides = AR.table_sides(B, S)
        assert {AR.mode_of(s, S) for s in sides} == {0, 1, 2}
        turns.add(len(AR.split_of(sides, S, 4, K)))
        l, e = AR.regimes(sides, S, nwave, K)
        for m in l:
            lens[m] |= l[m]
    assert turns == {1, 2, 3}                                                # one table, one image past it, two tables and one image
    assert lens[0] == {0, 1, 2, 3, 4} and lens[1] == {0, 1, 2, 3, 4}, lens
    rects = [AR.cutout_rect(S, *c) for c in AR.cutout_edges(S)]
    widths = {w for _h, w in rects}
    assert {0, 1, S - 1, S} <= widths and (S, S) in rects
    assert any(h & 1 and w & 1 and p % 2 == 0 for p, h, w in AR.cutout_edges(S))
    for b, (i, j, h, w) in enumerate(AR.boxes_for([2 * S, S, S // 2] * 12, *AR.grid_of(S))):
        assert i % 2 == 0 and j % 2 == 0 and i + h <= AR.grid_of(S)[0] and j + w <= AR.grid_of(S)[1]
    bx = AR.boxes_for([S] * 40, *AR.grid_of(S))
    Hy, Wy = AR.grid_of(S)
    assert any(i + h == Hy for i, j, h, w in bx) and any(j + w == Wy for i, j, h, w in bx) and any(i == 0 for i, *_ in bx)


# ================================================================================================== ops by raw arguments
def test_apply_raw_is_apply_op_for_every_listed_op():
    Y, Cc, quant = TA.synth(1, 28, 28, seed=11)
    Yd, Cd = O.dequantize(Y[0], Cc[0], quant[0])
    bank = CT._FilterBank()
    enc = [CT.encode_op(n, m, a, bank, 28) for n, m, a in TA.ALL_OPS]
    filt = np.stack([t.numpy() for t in bank.tables])
    for (n, m, a), e in zip(TA.ALL_OPS, enc):
        ry, rc = O.apply_op(Yd, Cd, n, m, a)
        gy, gc = AR.apply_raw(Yd, Cd, *e, filters=filt)
        assert np.array_equal(ry, gy) and np.array_equal(rc, gc), (n, m)


def test_oracle_matches_the_reference_on_flat_images(golden):
    """AutoContrast / AutoSaturation: kept at min = max = 0, else every DC 0; Equalize: every DC -1024."""
    g = golden("g24_flat.npz")
    seen = set()
    for k in range(int(g["ncases"])):
        name, (dy, dc) = str(g[f"case{k}_name"]), g[f"case{k}_dcs"]
        y, c = g["Y"].copy(), g["C"].copy()
        y[..., 0, 0] = dy
        c[..., 0, 0] = dc
        oy, oc = O.apply_op(y, c, name, 0.0)
        assert np.array_equal(oy, g[f"case{k}_Y"]) and np.array_equal(oc, g[f"case{k}_C"]), (k, name, dy, dc)
        ry, rc = AR.apply_raw(y, c, CT.OPS[name], 0.0, 0, 0, 0)
        assert np.array_equal(ry, oy) and np.array_equal(rc, oc)
        want = {"AutoContrast": 0, "AutoSaturation": int(dy), "Equalize": -1024}[name]
        assert (oy[..., 0, 0] == want).all(), (name, dy)
        seen.add((name, int(dy) == 0))
    assert len(seen) == 6                                  # each op on the zero and on the non-zero flat image


# ================================================================================================== seeded defects
def emu_case(S=28, B=3, nwave=64, gray=False):
    """One small mixed batch for the emulation: /2, identity and x2, all flipped (so that the flip defects bite)."""
    Y, Cc, quant = TA.synth(B, 64, 64, seed=2 if S == 28 else 8)
    sides = [2 * S, S, S // 2][:B]
    params = [dict(box=bx, flip=True) for bx in AR.boxes_for(sides, 64, 64)]
    return Y, (None if gray else Cc), quant, params


def check_emulated(oy, oc, Y, Cc, quant, params, S, raw=False, clamp_out=True):
    for b, p in enumerate(params):
        assert not (oy[b] == AR.UNWRITTEN).any() and not (oc[b] == AR.UNWRITTEN).any(), f"image {b}: elements never written"
        AR.check_image(oy[b], oc[b], Y[b], None if Cc is None else Cc[b], quant[b], p["box"], p["flip"], S, A16, raw, clamp_out,
                       f"image {b}")


@pytest.mark.parametrize("S", [28, 32])
def test_the_emulation_without_a_defect_is_accepted(S):
    Y, Cc, quant, params = emu_case(S)
    oy, oc = AR.emulate_k1(Y, Cc, quant, params, S, nwave=64, k=K)
    check_emulated(oy, oc, Y, Cc, quant, params, S)


@pytest.mark.parametrize("defect", [d for d in AR.DEFECTS_K1 if d != "packed_b0"])
def test_kernel1_defects_are_rejected(defect):
    Y, Cc, quant, params = emu_case(28)
    oy, oc = AR.emulate_k1(Y, Cc, quant, params, 28, nwave=64, k=K, defect=defect)
    with pytest.raises(AssertionError):
        check_emulated(oy, oc, Y, Cc, quant, params, 28)
    if defect == "lsb3":
        # the old bar accepts it: <= 1 LSB everywhere, fewer than 6 % of the coefficients differ
        gy, _ = AR.emulate_k1(Y, Cc, quant, params, 28, nwave=64, k=K)
        assert AR.old_bar(oy[0], gy[0]) and not np.array_equal(oy[0], gy[0])
        assert 0.02 < (oy[0] != gy[0]).mean() < 0.04


def test_packed_offsets_advanced_in_the_second_table_turn_are_rejected():
    Y8, C8, q8 = TA.synth(8, 64, 64, seed=9)
    B = AR.MAXB + 1
    idx = np.arange(B) % 8
    sides = AR.table_sides(B, 28)
    boxes = AR.boxes_for(sides, 64, 64)
    order = list(range(B))[::-1]
    packed = AR.pack_boxes([Y8[i] for i in idx], [C8[i] for i in idx], boxes, order, gap=64)
    # only the images of interest are emulated (513 images would be the same statement 513 times): the first image of the second
    # table turn, and one of the first turn as the control
    for b in (3, AR.MAXB):
        sub = [dict(box=boxes[b], flip=bool(b & 1))]
        args = (Y8[idx[b]][None], C8[idx[b]][None], q8[idx[b]][None])
        pk = (packed[0], packed[1], packed[2][b:b + 1], packed[3][b:b + 1])
        for defect in (None, "packed_b0"):
            oy, oc = AR.emulate_k1(*args, sub, 28, nwave=64, k=K, packed=pk, first=b, defect=defect)
            if defect and b >= AR.MAXB:
                with pytest.raises(AssertionError):
                    check_emulated(oy, oc, *args, sub, 28)
            else:
                check_emulated(oy, oc, *args, sub, 28)


OPS_DEFECTS = {
    # defect -> (first op as raw arguments, what the input must hold)
    "chroma_shift_trunc": ("raw", 9, 0.0, -5, 0, 0),          # an odd luma shift: -5 // 2 = -3, truncation gives -2
    "cutout_last_block": ("raw", 8, 0.0, 2, 7, 9),
    "rot_unclamped": ("raw", 11, 0.0, 1, 0, 0),
    "raw_no_entry_clamp": ("raw", 8, 0.0, 2, 7, 9),
}


@pytest.mark.parametrize("defect", AR.DEFECTS_K2)
def test_kernel2_defects_are_rejected(defect):
    Y, Cc, quant = TA.synth(1, 28, 28, seed=12)
    Yd, Cd = O.dequantize(Y[0], Cc[0], quant[0])
    Yd[0, 3, 4] = -1024
    Yd[0, 5, 6] = 1016
    if defect == "raw_no_entry_clamp":                       # an image that enters unclamped
        Yd, Cd = (Yd.astype(np.int32) * 3).astype(np.int16), (Cd.astype(np.int32) * 5).astype(np.int16)
        assert Yd.max() > 1016 and Cd.min() < -1024
    op = OPS_DEFECTS[defect]
    want = AR.expected_ops(Yd, Cd, [op])
    good = AR.emulate_ops(Yd, Cd, [op[1:]], clamped=True)
    assert np.array_equal(good[0], want[0]) and np.array_equal(good[1], want[1])
    bad = AR.emulate_ops(Yd, Cd, [op[1:]], clamped=True, defect=defect)
    assert not (np.array_equal(bad[0], want[0]) and np.array_equal(bad[1], want[1])), defect
