"""References, acceptance rules and a defect-seedable emulation of the DCT augment stage (csrc/augment.hip with
csrc/augment_body.inc), used by tests/test_augment_edges.py (GPU) and tests/test_augment_edges_cpu.py.  A plain module.

KERNEL 1 (de-quantise, clamp, crop, resize, flip, entry clamp) against fp64.  The int16 product with wrap-around and the clamp
(none in raw mode) are integer work and are done in integers.  The resize is then, per output coefficient,

    /2:  Z = A8 . X . A8^T / 2       X: the 2 x 2 input blocks as one 16 x 16 matrix, A8 = rows 0..7 of the conversion matrix
    x2:  Y = A8^T . (2 P) . A8        P: one input block, 16 x 16 out = 2 x 2 output blocks

evaluated in float64 ON THE fp32-VALUED MATRIX THE KERNEL IS HANDED (`raw`), together with the same expression on absolute values
(`mag`).  The kernel evaluates both products as fp32 FMA chains.  The window e, term by term (u = 2^-24, the unit roundoff):

  - the int16 -> fp32 conversions of X are exact (|x| < 2^24), and so are the factors 2 (x2, on the way in) and 1/2 (/2, on the way
    out): powers of two;
  - first product: every element is a chain of n1 FMAs, one rounding each: |fl(T) - T| <= n1 u |A8| |X|  (to first order);
  - second product: a chain of n2 FMAs over the computed T: n2 u |fl(T)| |A8| of its own plus the first error carried through
    |A8|: together (n1 + n2) u mag;
  - n1 = n2 = 16 for /2 (16-term inner products), 8 for x2 (P's other rows and columns are structural zeros: the kernel does
    not even multiply them);
  - two more units: one for the scale and one for the float -> int conversion.  Both are exact in the kernel; the two units are
    what covers the second-order terms ((n1 + n2)^2 / 2 u^2 mag << 2 u mag) that "to first order" dropped.

      e = (n1 + n2 + 2) u mag

A stored coefficient is ACCEPTED iff it equals finish(n) for an integer n = rint(t) with |t - raw| <= e, i.e. rint(raw - e) <= n <=
rint(raw + e) (rint is monotone), where finish() is int16 wrap, the flip (block columns mirrored, odd columns negated with int16
wrap) and the output clamp.  Where the interval holds one integer the check is bit exact; where it holds two (a tie inside the
window) either passes.  The identity resize has e = 0: bit exact everywhere.  The SHARE of coefficients with two admissible values
is a condition of the check, not a measurement: at most TIE_CAP (8 % for /2 -- the even/even frequencies of a /2 block are
quarter-integers of four input coefficients, 16 of 64 positions, a quarter of them at .5 -- and 0.1 % for x2).

KERNEL 2 (the op chain, ToRange) is bit exact in int16, fp32 and bf16 against oracle.dct_np.apply_op applied to kernel 1's OWN int16
output (read back with out_dtype 2 and nops 0): a resize tie can neither hide nor be blamed for anything in the op chain.  Ops
given as raw rgbnm_aug_params go through apply_raw(), the same oracle primitives keyed by the ABI's arguments (pinned to apply_op
on the CPU for every entry of test_augment.ALL_OPS).

WORK SPLIT: work_split() restates dct_resize_kernel's arithmetic (cost prefix table, equal shares, items whose START falls into a
share) in plain Python: per wave the list of (image, j0, j1) visits.

EMULATION: emulate_k1 / emulate_ops rebuild the stage in numpy from the fp32 oracle, item by item along work_split(), with one
seedable defect each: the CPU file runs them through the same check functions and every defect must be rejected.
"""
import os
import re

import numpy as np

from oracle import dct_np as O

CMIN, CMAX = O.CMIN, O.CMAX
U = 2.0 ** -24
CHAIN = {0: (16, 16), 2: (8, 8)}          # FMA-chain lengths (n1, n2) per resize mode
TIE_CAP = {0: 0.08, 2: 0.001}            # admissible share of two-valued coefficients per resize mode
MAXB = 512                               # images per cost prefix table (RESIZE_MAXB)
I16_CANARY = 0x7FC5                      # kernel_check's 16-bit canary read as an integer: 32709, outside [CMIN, CMAX]
UNWRITTEN = 31111                        # the emulation's "never written" value


# ----------------------------------------------------------------------------------------------------- geometry, work split
def mode_of(side, S):
    """0: /2, 1: identity, 2: x2 (augment_body.inc mode_of)."""
    return 0 if side == 2 * S else (1 if side == S else 2)


def units(S):
    return S * S + 2 * (S // 2) ** 2


def items_of(mode, S):
    return units(S) // (2, 8, 4)[mode]


def weights():
    """(AUG_K_HALF, AUG_K_ID, AUG_K_DBL): the per-item cost weights, read from the defaults of csrc/augment_body.inc."""
    import rgb_no_more_amd as rg
    src = open(os.path.join(os.path.dirname(rg.__file__), "csrc", "augment_body.inc")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("AUG_K_HALF", "AUG_K_ID", "AUG_K_DBL"))


def cost_prefix(modes, S, k):
    """launch()'s exclusive prefix sums of the images' costs (items x weight)."""
    pfx = [0]
    for m in modes:
        pfx.append(pfx[-1] + items_of(m, S) * k[m])
    return pfx


def work_split(pfx, nwave, modes, k):
    """dct_resize_kernel's share arithmetic: for every wave the list of its (image, j0, j1) visits."""
    B = len(pfx) - 1
    total = pfx[B]
    share, rem = divmod(total, nwave)
    head = np.asarray(pfx[:B])
    out = []
    for wave in range(nwave):
        lo = wave * share + min(wave, rem)
        hi = lo + share + (1 if wave < rem else 0)
        visits = []
        if lo < hi:
            b = int(np.searchsorted(head, lo, side="right")) - 1            # largest b with pfx[b] <= lo
            while b < B and pfx[b] < hi:
                kk = k[modes[b]]
                base, end = pfx[b], min(hi, pfx[b + 1])
                visits.append((b, (max(lo - base, 0) + kk - 1) // kk, (end - base + kk - 1) // kk))
                b += 1
        out.append(visits)
    return out


def split_of(sides, S, nwave, k):
    """work_split() of a batch given by its crop sides, one prefix table per MAXB images as launch() loops: a list of
    (first image of the turn, modes of the turn, visits per wave)."""
    turns = []
    for b0 in range(0, len(sides), MAXB):
        modes = [mode_of(s, S) for s in sides[b0:b0 + MAXB]]
        turns.append((b0, modes, work_split(cost_prefix(modes, S, k), nwave, modes, k)))
    return turns


def regimes(sides, S, nwave, k):
    """What a batch reaches: per mode the set of visit lengths min(j1 - j0, 4), and whether some wave's share starts behind an
    image's last item start (j0 == j1)."""
    lens, empty = {0: set(), 1: set(), 2: set()}, False
    for _b0, modes, waves in split_of(sides, S, nwave, k):
        for visits in waves:
            for b, j0, j1 in visits:
                lens[modes[b]].add(min(j1 - j0, 4))
                empty |= j0 == j1
    return lens, empty


# ----------------------------------------------------------------------------------------------------- kernel 1, fp64
def wrap16(x):
    return (np.asarray(x, np.int64) + 32768) % 65536 - 32768


def dequant_int(coef, qtab, raw):
    """int16 x int16 -> int16 WITH wrap-around, then the clamp (none in raw mode), in integers."""
    w = wrap16(np.asarray(coef, np.int64) * np.asarray(qtab, np.int64))
    return w if raw else np.clip(w, CMIN, CMAX)


def gather2(x):
    """[C, H, W, 8, 8] -> [C, H/2, W/2, 16, 16]: 2 x 2 blocks as one matrix (dct_ops.py:519)."""
    C, H, W = x.shape[:3]
    return x.reshape(C, H // 2, 2, W // 2, 2, 8, 8).transpose(0, 1, 3, 2, 5, 4, 6).reshape(C, H // 2, W // 2, 16, 16)


def scatter2(t):
    """[C, H, W, 16, 16] -> [C, 2 H, 2 W, 8, 8]."""
    C, H, W = t.shape[:3]
    return np.ascontiguousarray(t.reshape(C, H, W, 2, 8, 2, 8).transpose(0, 1, 3, 2, 5, 4, 6).reshape(C, 2 * H, 2 * W, 8, 8))


def resize64(X, mode, A):
    """(raw, mag) of one cropped plane set X [C, h, w, 8, 8] (integers), float64 on the fp32-valued matrix A [16, 16]."""
    X = X.astype(np.float64)
    if mode == 1:
        return X, np.abs(X)
    A8 = np.asarray(A, np.float32).astype(np.float64)[:8]
    if mode == 0:
        f = lambda M, x: M @ gather2(x) @ M.T / 2.0              # noqa: E731
    else:
        f = lambda M, x: scatter2(M.T @ (2.0 * x) @ M)            # noqa: E731
    return f(A8, X), f(np.abs(A8), np.abs(X))


def k1_ref(Yq, Cq, quant, box, S, A, raw=False):
    """Kernel 1 up to the rounding, for one image: Yq [1, Hy, Wy, 8, 8], Cq [2, Hc, Wc, 8, 8] or None (grayscale: zero chroma),
    quant [3, 8, 8], box (i, j, h, w) in luma blocks.  -> mode, [(raw, mag) of Y [1, S, S, 8, 8], (raw, mag) of C [2, S/2, S/2, 8, 8]]."""
    i, j, h, w = box
    mode = mode_of(w, S)
    X = dequant_int(Yq[:, i:i + h, j:j + w], quant[0], raw)
    if Cq is None:
        XC = np.zeros((2, h // 2, w // 2, 8, 8), np.int64)
    else:
        XC = dequant_int(Cq[:, i // 2:i // 2 + h // 2, j // 2:j // 2 + w // 2], np.asarray(quant)[1:3, None, None], raw)
    return mode, [resize64(X, mode, A), resize64(XC, mode, A)]


def mirror(x, flip):
    return x[:, :, ::-1] if flip else x


def finish(n, flip, clamp_out):
    """What kernel 1 does to the rounded integer: int16 wrap, flip (block columns mirrored, odd columns negated with wrap), clamp."""
    v = wrap16(n)
    if flip:
        v = v[:, :, ::-1].copy()
        v[..., 1::2] = wrap16(-v[..., 1::2])
    return np.clip(v, CMIN, CMAX) if clamp_out else v


def window(raw, mag, mode):
    if mode == 1:
        return np.zeros_like(raw)
    n1, n2 = CHAIN[mode]
    return (n1 + n2 + 2) * U * mag


def check_k1(got, raw, mag, mode, flip, clamp_out, where, cap=True):
    """The acceptance rule on one plane set (got: the stored int16 [C, S, S, 8, 8]).  Returns (worst |n - raw| / (0.5 + e) over
    the accepted integers n, share of coefficients with two admissible integers); raises AssertionError on a coefficient that no
    admissible integer explains, or (cap) on a share above TIE_CAP."""
    e = window(raw, mag, mode)
    lo, hi = np.rint(raw - e).astype(np.int64), np.rint(raw + e).astype(np.int64)
    width = int((hi - lo).max())
    assert width <= 2, f"{where}: the window admits {width + 1} integers somewhere: not a rounding check any more"
    g = np.asarray(got).astype(np.int64)
    assert g.shape == raw.shape, (where, g.shape, raw.shape)
    ok = np.zeros(g.shape, bool)
    ratio = np.zeros(g.shape)
    raw_l, e_l = mirror(raw, flip), mirror(e, flip)
    for d in range(width + 1):
        n = np.minimum(lo + d, hi)
        m = (finish(n, flip, clamp_out) == g) & ~ok
        ratio = np.where(m, np.abs(mirror(n, flip) - raw_l) / (0.5 + e_l), ratio)
        ok |= m
    if not ok.all():
        bad = np.argwhere(~ok)
        first = [f"{tuple(int(v) for v in c)}: got {int(g[tuple(c)])} raw {float(raw_l[tuple(c)]):.6f} e {float(e_l[tuple(c)]):.2e}"
                 for c in bad[:6]]
        raise AssertionError(f"{where}: {len(bad)} of {g.size} coefficients outside the rule; " + "; ".join(first))
    share = float((hi > lo).mean())
    if cap and mode != 1:
        assert share <= TIE_CAP[mode], f"{where}: {100 * share:.3f} % of the coefficients have two admissible values (cap " \
                                       f"{100 * TIE_CAP[mode]} %): the inputs do not test the rounding"
    return float(ratio.max()), share


def check_image(gotY, gotC, Yq, Cq, quant, box, flip, S, A, raw, clamp_out, where, cap=True):
    """check_k1 on both plane sets of one image; gray (Cq None): the chroma must be exactly zero.  -> mode, worst, (shareY, shareC)."""
    mode, ((ry, my), (rc, mc)) = k1_ref(Yq, Cq, quant, box, S, A, raw)
    wy, sy = check_k1(np.asarray(gotY).reshape(ry.shape), ry, my, mode, flip, clamp_out, where + " Y", cap)
    if Cq is None:
        assert not np.asarray(gotC).any(), f"{where}: chroma of a grayscale image is not exactly zero"
        return mode, wy, (sy, 0.0)
    wc, sc = check_k1(np.asarray(gotC).reshape(rc.shape), rc, mc, mode, flip, clamp_out, where + " C", cap)
    return mode, max(wy, wc), (sy, sc)


def old_bar(got, ref_i16):
    """The bar of tests/test_augment.py before this file: <= 1 LSB everywhere and fewer than 6 % of the coefficients differ (its
    third clause, exactness outside a 2e-3 window of a tie, ran on luma at size 28 only).  True: accepted."""
    d = np.abs(np.asarray(got, np.int64) - np.asarray(ref_i16, np.int64))
    return bool(d.max() <= 1 and (d > 0).mean() < 0.06)


# ----------------------------------------------------------------------------------------------------- kernel 2
def brightness_raw(Y, fm):
    out = Y.copy()
    dc = out[:, :, :, 0, 0].astype(np.float32)
    s = int(np.abs(out[:, :, :, 0, 0].astype(np.int64)).sum())           # exact integer sum, as the kernel's reduction
    out[:, :, :, 0, 0] = np.rint(dc + (np.float32(s) / np.float32(dc.size)) * np.float32(fm)).astype(np.int16)
    return out


def apply_raw(Y, C, op, fmag, a0, a1, a2, filters=None, clip=True, defect=None):
    """One op by its ABI arguments (include/rgbnm.h RGBNM_OP_*), built from the oracle's primitives, with the per-op clamp.
    Y [1, S, S, 8, 8], C [2, S/2, S/2, 8, 8] int16.  defect: see DEFECTS."""
    Y, C = Y.copy(), C.copy()
    if op == 0:
        pass
    elif op == 1:
        Y = O.autocontrast(Y)
    elif op == 2:
        assert a1 == round(2040 / 2 ** a0) + 1, "Posterize: iarg1 is the table length of iarg0"
        Y, C = O.posterize(Y, a0), O.posterize(C, a0)
    elif op == 3:
        dc = Y[:, :, :, 0, 0].astype(np.int64)
        Y[:, :, :, 0, 0] = np.where(dc < 0, wrap16(dc + wrap16(a0)), dc).astype(np.int16)          # int16 add, wraps
    elif op == 4:
        C = O.contrast(C, np.float32(fmag))
    elif op == 5:
        Y = O.contrast(Y, np.float32(fmag))
    elif op == 6:
        Y = brightness_raw(Y, fmag)
    elif op in (7, 15):
        F = np.asarray(filters, np.float32).reshape(-1, 8, 8)[a0]
        Y = np.rint(np.clip(Y.astype(np.float32) * F, np.float32(CMIN), np.float32(CMAX))).astype(np.int16)
    elif op == 8:
        if defect == "cutout_last_block":           # row index off by one at the rectangle's last block: that block is missed
            keepY, keepC = Y.copy(), C.copy()
        Y, C = O.cutout(Y, a0, a1, a2), O.cutout(C, a0 // 2, a1 // 2, a2 // 2)
        if defect == "cutout_last_block":
            for T, K, (p, ch, cw) in ((Y, keepY, (a0, a1, a2)), (C, keepC, (a0 // 2, a1 // 2, a2 // 2))):
                S = T.shape[1]
                r, c = S - max(0, ch - p) - 1, S - max(0, S - cw - p) - 1           # last row / column of the rectangle
                if r >= max(0, S - ch - p) and c >= max(0, cw - p):
                    T[:, r, c] = K[:, r, c]
    elif op in (9, 10):
        shC = int(a0 / 2) if defect == "chroma_shift_trunc" else a0 // 2
        d = "W" if op == 9 else "H"
        Y, C = O.translate(Y, a0, d), O.translate(C, shC, d)
    elif op == 11:
        Y, C = O.rotate90(Y, a0), O.rotate90(C, a0)
        if defect == "rot_unclamped":
            return np.ascontiguousarray(Y), np.ascontiguousarray(C)
    elif op == 12:
        C = O.autocontrast(C)
    elif op == 13:
        C = C * 0
    elif op == 14:
        C[0 if a0 else 1] *= 0
    elif op == 16:
        Y, C = wrap16(-Y.astype(np.int64)).astype(np.int16), wrap16(-C.astype(np.int64)).astype(np.int16)
    elif op == 17:
        mask = Y[:, :, :, 0, 0] > a0
        Y[mask] = wrap16(-Y[mask].astype(np.int64)).astype(np.int16)
        cm = np.tile(mask[:, ::2, ::2], (2, 1, 1))
        C[cm] = wrap16(-C[cm].astype(np.int64)).astype(np.int16)
    elif op == 18:
        for T in (Y, C):
            dc = T[..., 0, 0].copy()
            T[...] = np.rint(T.astype(np.float32) * np.float32(fmag)).astype(T.dtype)
            T[..., 0, 0] = dc
    elif op == 19:
        Y = O.equalize(Y)
    else:
        raise ValueError(op)
    if not clip:
        return np.ascontiguousarray(Y), np.ascontiguousarray(C)
    return np.ascontiguousarray(np.clip(Y, CMIN, CMAX)), np.ascontiguousarray(np.clip(C, CMIN, CMAX))


def expected_ops(Y, C, ops, filters=None):
    """The op chain on kernel 1's own int16 output.  An op is (name, magnitude, aux) -> oracle.dct_np.apply_op, or
    ("raw", id, fmag, iarg0, iarg1, iarg2) -> apply_raw."""
    for o in ops:
        Y, C = apply_raw(Y, C, *o[1:], filters=filters) if o[0] == "raw" else O.apply_op(Y, C, *o)
    return Y, C


def to_out(x, out_dtype):
    """int16 coefficients -> the stage's output in out_dtype ('i16' | 'f32' | 'bf16'); bf16 is returned as its fp32 value."""
    if out_dtype == "i16":
        return x
    r = O.to_range(x)
    if out_dtype == "f32":
        return r
    import torch
    return torch.from_numpy(r).bfloat16().float().numpy()


def guarded_i16(n, device="cuda"):
    """kernel_check.guarded for an int16 vector of n elements: the canary is the integer I16_CANARY (outside the clamp range; a
    test whose output is not clamped asserts that its expected output does not hold it)."""
    import torch
    import kernel_check as KC
    g = KC.guarded(n, None, torch.int16, device=device)
    assert g.canary == I16_CANARY
    return g


# ----------------------------------------------------------------------------------------------------- emulation with defects
DEFECTS_K1 = ("lsb3", "flip_even", "flip_chroma_nomirror", "item_dropped", "item_stale", "packed_b0")
DEFECTS_K2 = ("chroma_shift_trunc", "cutout_last_block", "raw_no_entry_clamp", "rot_unclamped")


def item_units(mode, S, j):
    """Output units (block numbers in [Y | Cb | Cr] order, before the flip) of item j."""
    if mode == 0:
        return [2 * j, 2 * j + 1]
    if mode == 1:
        return list(range(8 * j, 8 * j + 8))
    SYI, SCI = S // 2, S // 4
    if j < SYI * SYI:
        base, Sp, iy, ix = 0, S, j // SYI, j % SYI
    else:
        u2 = j - SYI * SYI
        pl, u3 = u2 // (SCI * SCI), u2 % (SCI * SCI)
        base, Sp, iy, ix = S * S + pl * (S // 2) ** 2, S // 2, u3 // SCI, u3 % SCI
    return [base + (2 * iy + r) * Sp + 2 * ix + s for r in (0, 1) for s in (0, 1)]


def pack_boxes(Yq, Cq, boxes, order, gap):
    """Host-cropped input as loader.DCTBatchLoader(crop_on_host=True) lays it out, but in the order `order` and with `gap`
    elements between boxes: flat Y, flat C, y_off[B], c_off[B] (element offsets; not monotonic in b)."""
    B = len(boxes)
    fy, fc, yoff, coff = [], [], [0] * B, [0] * B
    ny = nc = 0
    for b in order:
        i, j, h, w = boxes[b]
        fy += [np.full(gap, -21846, np.int16), np.ascontiguousarray(Yq[b][0, i:i + h, j:j + w]).reshape(-1)]
        yoff[b] = ny + gap
        ny += gap + h * w * 64
        if Cq is not None:
            fc += [np.full(gap, -21846, np.int16),
                   np.ascontiguousarray(Cq[b][:, i // 2:i // 2 + h // 2, j // 2:j // 2 + w // 2]).reshape(-1)]
            coff[b] = nc + gap
            nc += gap + 2 * (h // 2) * (w // 2) * 64
    return (np.concatenate(fy), np.concatenate(fc) if Cq is not None else None, np.asarray(yoff, np.int64), np.asarray(coff, np.int64))


def emulate_k1(Yq, Cq, quant, params, S, raw=False, clamp_out=True, nwave=4096, k=(9, 8, 12), defect=None, packed=None, first=0):
    """Kernel 1 in numpy: the fp32 oracle's resize per image, written item by item along work_split().  Yq [B, 1, Hy, Wy, 8, 8],
    Cq [B, 2, Hc, Wc, 8, 8] or None, quant [B, 3, 8, 8], params: dicts with box and flip.  packed: (flatY, flatC, yoff, coff) to
    read the boxes from instead; first: the place of params[0] in the whole batch (a slice of a longer batch is emulated on its
    own).  -> outY [B, 1, S, S, 8, 8], outC [B, 2, S/2, S/2, 8, 8] int64 (UNWRITTEN where no item wrote)."""
    B, SC = len(params), S // 2
    rng = np.random.default_rng(5)
    oy, oc = np.zeros((B, 1, S, S, 8, 8), np.int64), np.zeros((B, 2, SC, SC, 8, 8), np.int64)
    sides = [p["box"][3] for p in params]
    owner = {}
    for b0, modes, waves in split_of(sides, S, nwave, k):
        for wave, visits in enumerate(waves):
            for b, j0, j1 in visits:
                for j in range(j0, j1):
                    owner.setdefault(b0 + b, []).append((j, wave, j == j0 and j0 > 0))
    for b, p in enumerate(params):
        i, j, h, w = p["box"]
        mode = mode_of(w, S)
        if packed is not None:
            fy, fc, yoff, coff = packed
            sh = ((first + b) // MAXB * MAXB) if defect == "packed_b0" else 0           # offsets advanced once more by the turn's first image
            yo, co = int(yoff[b]) + sh * (h * w * 64), int(coff[b]) + sh * (2 * (h // 2) * (w // 2) * 64)
            idx = (yo + np.arange(h * w * 64)) % len(fy)
            Xq = fy[idx].reshape(1, h, w, 8, 8)
            Cc = None if fc is None else fc[(co + np.arange(2 * (h // 2) * (w // 2) * 64)) % len(fc)].reshape(2, h // 2, w // 2, 8, 8)
        else:
            Xq = Yq[b][:, i:i + h, j:j + w]
            Cc = None if Cq is None else Cq[b][:, i // 2:i // 2 + h // 2, j // 2:j // 2 + w // 2]
        X = dequant_int(Xq, quant[b][0], raw).astype(np.int16)
        XC = np.zeros((2, h // 2, w // 2, 8, 8), np.int16) if Cc is None else \
            dequant_int(Cc, np.asarray(quant[b])[1:3, None, None], raw).astype(np.int16)
        planes = []
        for T, Sp in ((X, S), (XC, SC)):
            r32 = O.resize_raw(T, Sp, np.float32).astype(np.float64)
            n = np.rint(r32).astype(np.int64)
            if defect == "lsb3" and mode != 1:           # + 1 on 3 % of the coefficients, all of them well away from a tie
                far = np.abs(r32 - np.floor(r32) - 0.5) > 0.2
                n = n + (far & (rng.random(n.shape) < 0.03))
            planes.append(n)
        blocks = np.concatenate([planes[0].reshape(-1, 8, 8), planes[1].reshape(-1, 8, 8)])          # [UNITS, 8, 8] before the flip
        done = np.full(blocks.shape, UNWRITTEN, np.int64)
        prev = None
        for jj, _wave, first_of_late_visit in sorted(owner.get(b, [])):
            us = item_units(mode, S, jj)
            if first_of_late_visit and defect == "item_dropped":
                prev = us
                continue
            src = prev if (first_of_late_visit and defect == "item_stale" and prev is not None) else us
            done[us] = blocks[src]
            prev = us
        ny = S * S
        for T, out, flipc in ((done[:ny].reshape(1, S, S, 8, 8), oy, True), (done[ny:].reshape(2, SC, SC, 8, 8), oc, False)):
            if p["flip"] and defect == "flip_even":
                v = wrap16(T)[:, :, ::-1].copy()
                v[..., 0::2] = wrap16(-v[..., 0::2])
                v = np.clip(v, CMIN, CMAX) if clamp_out else v
            elif p["flip"] and defect == "flip_chroma_nomirror" and not flipc:
                v = wrap16(T).copy()
                v[..., 1::2] = wrap16(-v[..., 1::2])
                v = np.clip(v, CMIN, CMAX) if clamp_out else v
            else:
                v = finish(T, p["flip"], clamp_out)
            out[b] = np.where(mirror(T, p["flip"]) == UNWRITTEN, UNWRITTEN, v)
    return oy, oc


def emulate_ops(Y, C, ops_raw, clamped, filters=None, defect=None):
    """Kernel 2's op chain on kernel 1's output (int16), ops as (id, fmag, iarg0, iarg1, iarg2).  clamped: the image entered
    clamped (entry_clamp bit 0); otherwise ONE full clamp after the first op.  Defect raw_no_entry_clamp: the image is taken as
    clamped although kernel 1 did not clamp it, so only what an op writes is clamped."""
    for o in ops_raw:
        before = (Y, C)
        if defect == "raw_no_entry_clamp":
            uy, uc = apply_raw(Y, C, *o, filters=filters, clip=False)
            Y = np.where(uy != before[0], np.clip(uy, CMIN, CMAX), before[0]).astype(np.int16)
            C = np.where(uc != before[1], np.clip(uc, CMIN, CMAX), before[1]).astype(np.int16)
        else:
            Y, C = apply_raw(Y, C, *o, filters=filters, defect=defect)
    return Y, C


# ----------------------------------------------------------------------------------------------------- shared case lists
def grid_of(S):
    """Luma grid (Hy, Wy) of the batch cases: non-square for the 28-grid, 64 x 64 for the 32-grid (whose /2 box is the whole grid)."""
    return (60, 64) if S == 28 else (64, 64)


def boxes_for(sides, Hy, Wy):
    """Even box corners that sweep the grid with the image index, far edges (crop_i + crop_h == Hy) and the origin included."""
    out = []
    for b, s in enumerate(sides):
        ni, nj = (Hy - s) // 2 + 1, (Wy - s) // 2 + 1
        out.append((2 * ((3 * b + 1) % ni) if ni > 1 else 0, 2 * ((5 * b + nj - 1) % nj) if nj > 1 else 0, s, s))
    return out


def small_cases(S):
    """(name, crop sides): B in {1, 2, 3, 5, 8} of each mode alone, and one batch with the three modes mixed."""
    out = [(f"{nm}-B{B}", [side] * B) for nm, side in (("half", 2 * S), ("ident", S), ("dbl", S // 2)) for B in (1, 2, 3, 5, 8)]
    return out + [("mixed-B8", [2 * S, S, S // 2, 2 * S, S, S, S // 2, 2 * S])]


def table_sides(B, S):
    """Mixed modes for the prefix-table cases, roughly the sampler's mix (half /2, a third identity, the rest x2)."""
    r = np.random.default_rng(B + S).random(B)
    return [2 * S if v < 0.5 else (S if v < 0.85 else S // 2) for v in r]


def table_boxes(sides, Hy, Wy):
    """Four box places per crop side (the place follows b % 4): with eight source images the batch holds a few hundred distinct
    (image, box, flip) combinations, each checked against fp64 once, and every image is compared with its combination's bits."""
    bx = {s: boxes_for([s] * 4, Hy, Wy) for s in set(sides)}
    return [bx[s][b % 4] for b, s in enumerate(sides)]


TABLE_BATCHES = (512, 513, 1025)

# Cutout (pad, centre h, centre w) in luma blocks, per output grid S: the four corners and the last block with pad 0 and 2, a pad
# of S and beyond (the whole image: S * S = 1024 luma blocks at S = 32), rectangle widths 1, S - 1 and S, an odd centre with an
# even pad (the chroma halving)
def cutout_edges(S):
    L = S - 1
    return [(p, h, w) for p in (0, 2) for h, w in ((0, 0), (0, L), (L, 0), (L, L))] + \
        [(S, S // 2, S // 2), (S + 6, 0, L), (2 * S, L, 0),
         (1, 0, 0), (1, 0, L),                    # width 1 (columns [0, 1) / [L - 1 .. ) clipped) -- odd pad: the ABI takes it
         (2, 1, 1), (2, 7, 9),                    # odd centres, even pad
         (S // 2, 0, S // 2 - 1),                 # width S - 1: columns [0, S - 1)
         (S // 2, L, S // 2)]                     # width S: columns [0, S)


def cutout_rect(S, pad, ch, cw):
    """(rows, columns) of the luma rectangle, as the kernel and the oracle clip it."""
    lower, upper = max(0, ch - pad), max(0, S - ch - pad)
    left, right = max(0, cw - pad), max(0, S - cw - pad)
    return max(0, S - lower - upper), max(0, S - right - left)
