"""Element-wise tests of the DCT augment stage (csrc/augment.hip with csrc/augment_body.inc, both instantiations: 28- and 32-block
output grids) at the C ABI (include/rgbnm.h: rgbnm_dct_augment_ex, rgbnm_dct_augment_packed), against the references and rules
of tests/augment_ref.py (read its docstring first; tests/test_augment_edges_cpu.py proves on the CPU that the rules admit a correct
fp32 evaluation, that the case lists reach the regimes they claim and that the seeded defects are rejected).

Every run: guarded outputs (kernel_check.guarded; the int16 output with an integer canary), a guarded workspace of exactly
rgbnm_dct_augment_workspace_ex(B, size) bytes, and a second run on inputs whose every coefficient OUTSIDE the crop boxes (packed
input: the gaps between the boxes) holds another pattern -- the outputs must be the same bits.

Kernel 1 (nops 0, int16 out) is checked per coefficient against fp64 with the derived window (bit exact wherever the window holds
one integer; the share of two-valued coefficients is capped per case); kernel 2 bit for bit in int16, fp32 and bf16 against
oracle.dct_np.apply_op on kernel 1's own int16 output.  Worst |n - raw| / (0.5 + e) per mode and the file's run time on one MI355X
are in DESIGN.md ("DCT augment stage, element-wise")."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_ref as AR
import kernel_check as KC
import test_augment as TA
from oracle import dct_np as O
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import dct_ops as dops
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EWORKSPACE = -1, -3
OUT = {"i16": (torch.int16, 2), "f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}
FILL = (-21846, 13107)                 # what lies outside the boxes in the first and in the second run
MODE_NAME = ("half", "ident", "dbl")
WORST = KC.Worst()
SHARES = {}


# ================================================================================================== harness
class Stage:
    """Per output grid: the parameter packer (TrainTransform_DCT.pack), its filter bank and the conversion matrix the kernel is handed."""

    def __init__(self, S):
        self.S = S
        self.t = CT.TrainTransform_DCT(size=S)
        A = dops.generate_conversion_matrix(8, 2).float().contiguous()
        self.A_np = A.numpy().copy()
        self.A = A.to(DEV)
        for kind, mag in (("MidfreqAug", 0.27), ("MidfreqAug", -0.27), ("Sharpness", 0.27), ("Sharpness", -0.27),
                          ("MidfreqAug", 0.9), ("Sharpness", -0.9)):
            self.t.bank.index(kind, mag)
        self.last_filter = {"MidfreqAug": len(self.t.bank.tables) - 2, "Sharpness": len(self.t.bank.tables) - 1}

    def pack(self, params):
        """TrainTransform_DCT.pack; an op ("raw", id, fmag, iarg0, iarg1, iarg2) is written into the struct as it is."""
        named = [dict(p, ops=[("Identity", 0.0, None) if o[0] == "raw" else o for o in p["ops"]]) for p in params]
        arr, nops = self.t.pack(named)
        for b, p in enumerate(params):
            for s, o in enumerate(p["ops"]):
                if o[0] == "raw":
                    arr[b].op[s], arr[b].fmag[s], arr[b].iarg0[s], arr[b].iarg1[s], arr[b].iarg2[s] = o[1:]
        return arr, nops

    def filters_np(self):
        return np.stack([t.numpy() for t in self.t.bank.tables])


_STAGES = {}


def stage(S):
    if S not in _STAGES:
        _STAGES[S] = Stage(S)
    return _STAGES[S]


def synth_grid(n, Hy, Wy, Hc, Wc, seed, gray=False):
    """test_augment.synth on a luma grid Hy x Wy with a chroma grid Hc x Wc >= Hy/2 x Wy/2."""
    Y, Cc, q = TA.synth(n, 2 * Hc, 2 * Wc, seed=seed, gray=gray)
    return np.ascontiguousarray(Y[:, :, :Hy, :Wy]), Cc, q


class Inputs:
    """A batch: image b is source image idx[b] (host numpy, device tensors), its crop box boxes[b].  Two variants of the device
    input that differ everywhere outside the boxes: whole grids (outside = the rest of the grid), or packed (outside = gaps of
    `gap` elements between the boxes, which lie in the order `order`: offsets neither monotonic nor a multiple of anything)."""

    def __init__(self, Y8, C8, q8, idx, boxes, packed=False, gap=200):
        self.Y8, self.C8, self.q8, self.idx, self.boxes, self.B = Y8, C8, q8, np.asarray(idx), boxes, len(idx)
        self.Hy, self.Wy = Y8.shape[2:4]
        self.Hc, self.Wc = C8.shape[2:4] if C8 is not None else (self.Hy // 2, self.Wy // 2)
        di = torch.as_tensor(self.idx, device=DEV)
        Yd = torch.from_numpy(Y8).to(DEV)[di].contiguous()
        Cd = None if C8 is None else torch.from_numpy(C8).to(DEV)[di].contiguous()
        self.qd = torch.from_numpy(q8).to(DEV)[di].contiguous()
        bx = torch.tensor(boxes, device=DEV)
        if not packed:
            def keep(H, W, div):
                r = torch.arange(H, device=DEV)[None, :, None]
                c = torch.arange(W, device=DEV)[None, None, :]
                i, j, h, w = [(bx[:, k] // div)[:, None, None] for k in range(4)]
                return ((r >= i) & (r < i + h) & (c >= j) & (c < j + w))[:, None, :, :, None, None]
            self.variants = []
            for f in FILL:
                fill = torch.tensor(f, dtype=torch.int16, device=DEV)
                if f == FILL[0]:
                    self.variants.append((Yd, Cd, None, None))
                else:
                    self.variants.append((torch.where(keep(self.Hy, self.Wy, 1), Yd, fill),
                                          None if Cd is None else torch.where(keep(self.Hc, self.Wc, 2), Cd, fill), None, None))
        else:
            order = np.random.default_rng(self.B).permutation(self.B)
            ny = sum(gap + h * w * 64 for _i, _j, h, w in boxes) + gap
            nc = sum(gap + 2 * (h // 2) * (w // 2) * 64 for _i, _j, h, w in boxes) + gap
            yoff, coff = np.zeros(self.B, np.int64), np.zeros(self.B, np.int64)
            fys = [torch.full((ny,), f, dtype=torch.int16, device=DEV) for f in FILL]
            fcs = [None if Cd is None else torch.full((nc,), f, dtype=torch.int16, device=DEV) for f in FILL]
            py = pc = 0
            for b in order:
                i, j, h, w = boxes[b]
                yoff[b], coff[b] = py + gap, pc + gap
                by = Yd[b, 0, i:i + h, j:j + w].reshape(-1)
                for fy in fys:
                    fy[py + gap:py + gap + by.numel()] = by
                py += gap + by.numel()
                n2 = 2 * (h // 2) * (w // 2) * 64
                if Cd is not None:
                    bc = Cd[b, :, i // 2:i // 2 + h // 2, j // 2:j // 2 + w // 2].reshape(-1)
                    for fc in fcs:
                        fc[pc + gap:pc + gap + n2] = bc
                pc += gap + n2
            assert (np.diff(yoff) < 0).any() or self.B < 8
            yo, co = torch.from_numpy(yoff).to(DEV), torch.from_numpy(coff).to(DEV)
            self.variants = [(fys[k], fcs[k], yo, co) for k in range(2)]

    def host(self, b):
        k = self.idx[b]
        return self.Y8[k], None if self.C8 is None else self.C8[k], self.q8[k]


class Prepared:
    """One call of the stage with guarded outputs and workspace; fire() makes the call and returns its code."""

    def __init__(self, st, inp, arr, nops, variant=0, entry=1, out="i16", short=0, filt=True, B=None, size=None, odt=None,
                 drop_coff=False):
        S, nB = st.S, inp.B
        dt, code = OUT[out]
        ny, nc = nB * S * S * 64, nB * 2 * (S // 2) ** 2 * 64
        mk = (lambda n: AR.guarded_i16(n)) if out == "i16" else (lambda n: KC.guarded(n, None, dt))
        self.gy, self.gc = mk(ny), mk(nc)
        wsb = L.lib().rgbnm_dct_augment_workspace_ex(nB, S)
        assert wsb == nB * AR.units(S) * 64 * 2
        self.gw = AR.guarded_i16(wsb // 2)                       # exactly the bytes the library asks for
        self.arr = arr
        self.pdev = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(DEV)
        f = st.t.bank.device_tensor(DEV) if filt else None
        Yd, Cd, yo, co = inp.variants[variant]
        self.keep = (f, Yd, Cd, yo, co, inp.qd)
        tail = (self.pdev.data_ptr(), C.cast(arr, C.c_void_p), st.A.data_ptr(), L.ptr(f), self.gy.t.data_ptr(),
                self.gc.t.data_ptr(), code if odt is None else odt, S if size is None else size, nB if B is None else B, inp.Hy,
                inp.Wy, inp.Hc, inp.Wc, entry, nops, self.gw.t.data_ptr(), wsb - short, L.stream())
        if yo is None:
            self.fn, self.args = L.lib().rgbnm_dct_augment_ex, (Yd.data_ptr(), L.ptr(Cd), inp.qd.data_ptr()) + tail
        else:
            self.fn = L.lib().rgbnm_dct_augment_packed
            self.args = (Yd.data_ptr(), L.ptr(Cd), yo.data_ptr(), None if drop_coff else co.data_ptr(), inp.qd.data_ptr()) + tail

    def fire(self):
        return self.fn(*self.args)

    def outputs(self):
        return tuple(g.t.float().cpu().numpy() if g.dtype == torch.bfloat16 else g.t.cpu().numpy() for g in (self.gy, self.gc))

    def untouched(self):
        return all(bool((g.raw == g.canary).all()) for g in (self.gy, self.gc, self.gw))


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def run(st, inp, arr, nops, where, written=True, **kw):
    """The stage on both variants of the input: code 0, guards intact, every output element written, same bits from both."""
    outs = []
    for v in range(2):
        p = Prepared(st, inp, arr, nops, variant=v, **kw)
        rc = p.fire()
        torch.cuda.synchronize()
        assert rc == 0, f"{where}: rgbnm error {rc}"
        p.gy.check(f"{where} outY", written=written)
        p.gc.check(f"{where} outC", written=written)
        p.gw.check(f"{where} workspace", written=written)
        outs.append(p.outputs())
    S = st.S
    for k, nm in ((0, "Y"), (1, "C")):
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), f"{where}: out{nm} depends on coefficients outside the crop boxes"
    return outs[0][0].reshape(inp.B, 1, S, S, 8, 8), outs[0][1].reshape(inp.B, 2, S // 2, S // 2, 8, 8)


def check_batch(st, inp, params, oy, oc, where, raw=False, clamp_out=True):
    """Every image against the fp64 rule.  Images that are the same (source image, box, flip) must hold the same bits as the first of
    them, which is checked per coefficient.  The two-valued shares are capped per case, mode and plane set."""
    first, shares, modes = {}, {}, set()
    for b, p in enumerate(params):
        key = (int(inp.idx[b]), tuple(p["box"]), bool(p["flip"]))
        if key in first:
            a = first[key]
            assert np.array_equal(oy[b], oy[a]) and np.array_equal(oc[b], oc[a]), f"{where}: image {b} differs from its twin {a}"
            continue
        first[key] = b
        Yh, Ch, qh = inp.host(b)
        mode, worst, (sy, sc) = AR.check_image(oy[b], oc[b], Yh, Ch, qh, p["box"], p["flip"], st.S, st.A_np, raw, clamp_out,
                                               f"{where} image {b} box {p['box']} flip {p['flip']}", cap=False)
        WORST(f"S{st.S}-{MODE_NAME[mode]}", worst)
        shares.setdefault((mode, "Y"), []).append(sy)
        shares.setdefault((mode, "C"), []).append(sc)
        modes.add(mode)
    for (mode, pl), v in shares.items():
        if mode != 1 and not (pl == "C" and inp.C8 is None):
            share = float(np.mean(v))
            SHARES[f"S{st.S}-{MODE_NAME[mode]}-{pl}"] = max(SHARES.get(f"S{st.S}-{MODE_NAME[mode]}-{pl}", 0.0), share)
            assert share <= AR.TIE_CAP[mode], f"{where}: two-valued share {100 * share:.3f} % of mode {mode} {pl} above its cap"
        elif mode == 1:
            assert max(v) == 0.0
    return modes


def report(title):
    WORST.report(title)
    print(f"[{title}] largest two-valued share per case: " + ", ".join(f"{k}={100 * v:.4f}%" for k, v in sorted(SHARES.items())))


def params_of(boxes, flips=None, ops=None):
    return [dict(box=bx, flip=bool(b & 1) if flips is None else bool(flips[b]), ops=[] if ops is None else ops[b])
            for b, bx in enumerate(boxes)]


def device_nwave():
    """Waves of kernel 1's grid: CUs x occupancy workgroups (4 per CU: __launch_bounds__(256, 4), 33 KB of LDS each) x 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * 4


@pytest.fixture(scope="module")
def sources():
    """Eight source images per (output grid): luma grid AR.grid_of(S), computed once and left unchanged."""
    out = {}
    for S in (28, 32):
        Hy, Wy = AR.grid_of(S)
        out[S] = synth_grid(8, Hy, Wy, Hy // 2, Wy // 2, seed=20 + S)
    return out


# ================================================================================================== kernel 1: work split
@pytest.mark.parametrize("S", [28, 32])
def test_small_batches_every_mode_alone_and_mixed(S, sources):
    st, (Y8, C8, q8), K, nwave = stage(S), sources[S], AR.weights(), device_nwave()
    Hy, Wy = AR.grid_of(S)
    lens, empty = {0: set(), 1: set(), 2: set()}, False
    for name, sides in AR.small_cases(S):
        boxes = AR.boxes_for(sides, Hy, Wy)
        params = params_of(boxes)
        inp = Inputs(Y8, C8, q8, np.arange(len(sides)), boxes)
        arr, _ = st.pack(params)
        oy, oc = run(st, inp, arr, 0, f"S{S} {name}")
        modes = check_batch(st, inp, params, oy, oc, f"S{S} {name}")
        assert modes == {AR.mode_of(s, S) for s in sides}
        l, e = AR.regimes(sides, S, nwave, K)
        for m in l:
            lens[m] |= l[m]
        empty |= e
    # on this device's grid the small batches give every wave a visit of 0, 1 or 2 items (the start-up wait counts) and some
    # wave a share that starts behind an image's last item start; 3 and >= 4 items: the prefix-table cases below
    assert {0, 1} <= lens[0] and {0, 1} <= lens[1] and empty, (nwave, lens, empty)
    for B in AR.TABLE_BATCHES:
        l, _ = AR.regimes(AR.table_sides(B, S), S, nwave, K)
        for m in l:
            lens[m] |= l[m]
    assert lens[0] == {0, 1, 2, 3, 4} and lens[1] == {0, 1, 2, 3, 4}, (nwave, lens)
    report(f"small batches S{S}")


@pytest.mark.parametrize("B,packed,S", [(512, False, 28), (512, True, 28), (513, False, 28), (513, True, 28), (1025, False, 28),
                                        (1025, True, 28), (513, False, 32), (513, True, 32)])
def test_prefix_table_loop_every_image_against_fp64(B, packed, S, sources):
    st, (Y8, C8, q8) = stage(S), sources[S]
    sides = AR.table_sides(B, S)
    boxes = AR.table_boxes(sides, *AR.grid_of(S))
    params = params_of(boxes, flips=[(b // 3) & 1 for b in range(B)])
    inp = Inputs(Y8, C8, q8, np.arange(B) % 8, boxes, packed=packed)
    arr, _ = st.pack(params)
    oy, oc = run(st, inp, arr, 0, f"S{S} B{B} packed={packed}")
    assert check_batch(st, inp, params, oy, oc, f"S{S} B{B} packed={packed}") == {0, 1, 2}
    report(f"prefix tables S{S} B{B} packed={packed}")


# ================================================================================================== kernel 1: geometry
GEOMETRY = {28: [(58, 62, 29, 31), (59, 61, 30, 31), (58, 62, 33, 36)],
            32: [(66, 70, 33, 35), (65, 67, 33, 34), (64, 64, 35, 40)]}


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("S", [28, 32])
def test_geometry_non_square_grids_larger_chroma_grids_and_edge_boxes(S, packed):
    """(Hy, Wy, Hc, Wc): a non-square grid; the shape the reader returns for an odd luma grid (libjpeg's component sizes:
    chroma = ceil(luma / 2) blocks, csrc/reader.c); a chroma grid larger than that.  Boxes at the origin and flush with the far
    edges (the largest even corner), in every mode, flipped and not."""
    st = stage(S)
    for g, (Hy, Wy, Hc, Wc) in enumerate(GEOMETRY[S]):
        Y8, C8, q8 = synth_grid(4, Hy, Wy, Hc, Wc, seed=40 + g)
        boxes = []
        for side in (2 * S, S, S // 2):
            fi, fj = (Hy - side) // 2 * 2, (Wy - side) // 2 * 2
            boxes += [(0, 0, side, side), (fi, fj, side, side), (0, fj, side, side), (fi, 0, side, side)]
        if Hy % 2 == 0:
            assert any(i + h == Hy for i, j, h, w in boxes) and any(j + w == Wy for i, j, h, w in boxes)
        params = params_of(boxes, flips=[(b >> 1) & 1 for b in range(len(boxes))])
        inp = Inputs(Y8, C8, q8, np.arange(len(boxes)) % 4, boxes, packed=packed)
        assert (inp.Hc, inp.Wc) == (Hc, Wc) and Hc >= (Hy + 1) // 2
        arr, _ = st.pack(params)
        oy, oc = run(st, inp, arr, 0, f"S{S} grid {Hy}x{Wy}/{Hc}x{Wc} packed={packed}")
        check_batch(st, inp, params, oy, oc, f"S{S} grid {Hy}x{Wy}/{Hc}x{Wc} packed={packed}")
    report(f"geometry S{S} packed={packed}")


# ================================================================================================== grayscale
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("S", [28, 32])
def test_grayscale_zero_chroma_in_every_mode(S, packed, sources):
    st, (Y8, _C8, q8) = stage(S), sources[S]
    sides = [2 * S, S, S // 2, 2 * S, S, S // 2]
    boxes = AR.boxes_for(sides, *AR.grid_of(S))
    ops = [[("Brightness", 0.27, None), ("Rotate90", 1.0, None)], [("Contrast", -0.27, None), ("TranslateX", 3.75, None)]] * 3
    params = params_of(boxes, ops=ops)
    inp = Inputs(Y8, None, q8, np.arange(6), boxes, packed=packed)          # CbCrq / Cpacked NULL (c_off given)
    arr, nops = st.pack(params)
    where = f"S{S} gray packed={packed}"
    ky, kc = run(st, inp, arr, 0, where)
    check_batch(st, inp, params, ky, kc, where)                               # chroma exactly zero before the ops
    assert not kc.any()
    zero = O.to_range(np.zeros(1, np.int16))[0]
    for out in ("i16", "f32", "bf16"):
        oy, oc = run(st, inp, arr, nops, f"{where} {out}", out=out)
        for b, p in enumerate(params):
            ey, ec = AR.expected_ops(ky[b], kc[b], p["ops"])
            assert np.array_equal(bits(oy[b]), bits(AR.to_out(ey, out))), (where, out, b)
            assert np.array_equal(bits(oc[b]), bits(AR.to_out(ec, out))), (where, out, b)
        if out == "f32":
            assert (oc == zero).all()                                       # to_range(0)


# ================================================================================================== entry modes
def outside(x):
    return bool((x > 1016).any() or (x < -1024).any())


def entry_inputs(S):
    """De-quantised values that leave [-1024, 1016] and wrap int16; luma DCs of image 2 (Equalize first) stay inside the range in
    every entry mode; image 3 de-quantises to -32768 somewhere (Invert first)."""
    Y, Cc, q = TA.synth(6, 40, 40, seed=50 + S)
    q = (q.astype(np.int32) * 9).astype(np.int16)
    Y[:, 0, 1::3, 2::5, 1, 1] = 12000
    Y[:, 0, ::4, 1::3, 3, 3] = -1024                   # x 27: wraps
    Y[:, 0, ::2, ::2, 5, 5] = -10                      # x 189: clamps to -1024 at an odd column: the flip's negation gives 1024
    Y[2, 0, :, :, 0, 0] = np.random.default_rng(3).integers(-37, 38, (40, 40))
    cands = np.arange(-32768, 32768)
    hit = cands[AR.wrap16(cands * int(q[3, 0, 2, 0])) == -32768]
    assert hit.size
    Y[3, 0, :, :, 2, 0] = hit[0]
    return Y, Cc, q


@pytest.mark.parametrize("S", [28, 32])
def test_entry_modes_times_number_of_ops(S):
    st = stage(S)
    Y8, C8, q8 = entry_inputs(S)
    prod = Y8.astype(np.int64) * q8[:, 0][:, None, None, None]
    w = AR.wrap16(prod)
    assert (w != prod).any() and (w > 1016).any() and (w < -1024).any()            # the inputs wrap, and leave the range
    sides = [S, S, S, S, S // 2, S]
    boxes = [(2, 4, S, S), (0, 0, S, S), (4, 2, S, S), (40 - S, 40 - S, S, S), (6, 8, S // 2, S // 2), (2, 2, S, S)]
    first = [("raw", 8, 0.0, 2, 7, 9), ("ChromaDrop", 0.0, True), ("Equalize", 0.0, None), ("Invert", 0.0, None),
             ("raw", 8, 0.0, 4, S - 1, 0), ("Rotate90", -1.0, None)]
    second = [("Rotate90", 1.0, None), ("Posterize", 2.0, None), ("TranslateY", -3.75, None), ("Grayscale", 0.0, None),
              ("Posterize", 4.0, None), ("Contrast", 0.27, None)]
    params = params_of(boxes, flips=[1, 0, 1, 0, 1, 1], ops=[[a, b] for a, b in zip(first, second)])
    inp = Inputs(Y8, C8, q8, np.arange(6), boxes)
    arr, _ = st.pack(params)
    for entry in (0, 1, 2, 3):
        raw, clamp_out = bool(entry & 2), bool(entry & 1)
        where = f"S{S} entry_clamp {entry}"
        ky, kc = run(st, inp, arr, 0, f"{where} nops 0", entry=entry, written=clamp_out)
        check_batch(st, inp, params, ky, kc, f"{where} nops 0", raw=raw, clamp_out=clamp_out)
        assert outside(ky) == (not clamp_out)
        if not clamp_out:
            assert (ky[0] == 1024).any() or raw                  # the flip's negation of -1024
            assert not (ky == AR.I16_CANARY).any() and not (kc == AR.I16_CANARY).any()
        if raw and not clamp_out:
            assert np.abs(ky[4].astype(np.int64)).max() > 1024          # raw mode after a x2 resize whose result leaves the range
            assert (ky[3] == -32768).any()
        for nops in (1, 2):
            outs = ("i16", "f32", "bf16") if (entry, nops) == (1, 2) else ("i16",)
            for out in outs:
                oy, oc = run(st, inp, arr, nops, f"{where} nops {nops} {out}", entry=entry, out=out)
                for b, p in enumerate(params):
                    ey, ec = AR.expected_ops(ky[b], kc[b], p["ops"][:nops])
                    if not clamp_out and (b in (0, 2) or (raw and b in (1, 4))):
                        # the first op wrote only a part: the rest left the range before it and is clamped after it
                        assert outside(ky[b]) or outside(kc[b]), (where, b)
                    assert np.array_equal(bits(oy[b]), bits(AR.to_out(ey, out))), (where, nops, out, b, "Y")
                    assert np.array_equal(bits(oc[b]), bits(AR.to_out(ec, out))), (where, nops, out, b, "C")
    report(f"entry modes S{S}")


# ================================================================================================== kernel 2
def ops_case(st, inp, params, where, outs=("i16", "f32", "bf16"), tweak=None):
    """Kernel 1's own output (nops 0, int16), then the op chain in every output type against apply_op / apply_raw on it."""
    arr, nops = st.pack(params)
    ky, kc = run(st, inp, arr, 0, f"{where} kernel 1")
    if tweak is not None:
        tweak(arr, params, ky, kc)
    filt = st.filters_np()
    exp = [AR.expected_ops(ky[b], kc[b], p["ops"], filters=filt) for b, p in enumerate(params)]
    for out in outs:
        oy, oc = run(st, inp, arr, nops, f"{where} {out}", out=out)
        for b, p in enumerate(params):
            assert np.array_equal(bits(oy[b]), bits(AR.to_out(exp[b][0], out))), (where, out, b, p["ops"], "Y")
            assert np.array_equal(bits(oc[b]), bits(AR.to_out(exp[b][1], out))), (where, out, b, p["ops"], "C")
    return ky, kc, exp


@pytest.mark.parametrize("S", [28, 32])
def test_every_op_after_every_resize(S, sources):
    st, (Y8, C8, q8) = stage(S), sources[S]
    n = len(TA.ALL_OPS)
    assert n == 33
    sides, ops = [], []
    for b in range(2 * n):
        op = TA.ALL_OPS[b % n]
        sides.append(2 * S if b < n else S // 2)
        ops.append([op, TA.ALL_OPS[(b * 7 + 3 + b // n) % n]])
    ops = [[(o[0], o[1], tuple(min(v, S - 2) for v in o[2]) if o[0] == "Cutout" else o[2]) for o in pair] for pair in ops]
    boxes = AR.boxes_for(sides, *AR.grid_of(S))
    params = params_of(boxes, ops=ops)
    inp = Inputs(Y8, C8, q8, np.arange(2 * n) % 8, boxes)
    ops_case(st, inp, params, f"S{S} every op after /2 and x2")


def edge_sources(S):
    """Images 0..5: synthetic, with -1024 and 1016 planted at odd rows and columns; 6: every DC zero; 7: every DC equal, not zero."""
    Y, Cc, q = TA.synth(8, 2 * S, 2 * S, seed=60 + S)
    Y[:, 0, ::3, ::2, 1, 3] = -600
    Y[:, 0, 1::3, ::2, 3, 1] = 600
    Y[:, 0, ::3, 1::2, 0, 0] = -600
    Y[6, 0, :, :, 0, 0], Cc[6, :, :, :, 0, 0] = 0, 0
    Y[7, 0, :, :, 0, 0], Cc[7, :, :, :, 0, 0] = 33, 7
    return Y, Cc, q


def edge_ops(S, st):
    """(raw op, source image or None, crop side or None): the argument edges of the issue, as raw rgbnm_aug_params."""
    L_ = S - 1
    out = [(("raw", 8, 0.0, p, h, w), None, None) for p, h, w in AR.cutout_edges(S)]
    for op in (9, 10):
        out += [(("raw", op, 0.0, sh, 0, 0), None, None) for sh in (2, -2, S - 2, -(S - 2), S, -S, S + 3, -(S + 3), -6, -3, -5, 3)]
    out += [(("raw", 11, 0.0, d, 0, 0), None, S) for d in (1, -1)]
    out += [(("raw", 2, 0.0, b, round(2040 / 2 ** b) + 1, 0), None, None) for b in range(9)]
    out += [(("raw", 3, 0.0, -32000, 0, 0), None, S), (("raw", 3, 0.0, 32767, 0, 0), None, S)]
    out += [(("raw", 17, 0.0, 0, 0, 0), None, S), (("raw", 17, 0.0, 0, 0, 0), None, 2 * S)]          # threshold set from kernel 1's DCs
    out += [(("raw", op, f, 0, 0, 0), None, None) for op in (18, 5, 4, 6) for f in (0.5, 1.5, -0.5)]
    out += [(("raw", 7, 0.0, st.last_filter["MidfreqAug"], 0, 0), None, None), (("raw", 15, 0.0, st.last_filter["Sharpness"], 0, 0), None, None)]
    out += [(("raw", op, 0.0, 0, 0, 0), img, S) for op in (1, 12, 19) for img in (6, 7)]
    return out


@pytest.mark.parametrize("S", [28, 32])
def test_op_argument_edges(S):
    st = stage(S)
    Y8, C8, q8 = edge_sources(S)
    cases = edge_ops(S, st)
    sides = [c[2] if c[2] is not None else (2 * S, S, S // 2)[b % 3] for b, c in enumerate(cases)]
    idx = [c[1] if c[1] is not None else b % 6 for b, c in enumerate(cases)]
    boxes = AR.boxes_for(sides, 2 * S, 2 * S)
    flips = [b & 1 if c[0][1] != 11 else 0 for b, c in enumerate(cases)]         # Rotate90: the planted -1024 stay at their odd columns
    params = params_of(boxes, flips=flips, ops=[[c[0], ("Identity", 0.0, None)] for c in cases])
    inp = Inputs(Y8, C8, q8, idx, boxes)
    sol = [b for b, c in enumerate(cases) if c[0][1] == 17]

    def tweak(arr, params, ky, kc):
        for b in sol:                    # Solarize: a threshold exactly equal to DCs that kernel 1 left in the image
            dcs = np.sort(ky[b][0, :, :, 0, 0].reshape(-1))
            thr = int(dcs[len(dcs) // 2])
            arr[b].iarg0[0] = thr
            params[b]["ops"][0] = ("raw", 17, 0.0, thr, 0, 0)
            assert (dcs == thr).any() and (dcs > thr).any()

    ky, kc, exp = ops_case(st, inp, params, f"S{S} op argument edges", tweak=tweak)
    for b, c in enumerate(cases):
        op, _f, a0 = c[0][1:4]
        Yk, (ey, ec) = ky[b], exp[b]
        if op == 11:       # the negation of -1024 leaves the range and is clamped
            assert (Yk[..., 1::2, :] == -1024).any() and (Yk[..., 1::2] == -1024).any() and (Yk == 1016).any() and ey.max() == 1016
        if op in (9, 10) and abs(a0) >= S:
            assert not ey.any() and not ec.any()
        if op == 8 and a0 >= S:
            assert not ey.any() and not ec.any()
        if op == 3 and a0 == -32000:
            assert (Yk[0, :, :, 0, 0] < -768).any()                   # the int16 sum wraps to a large positive value: 1016, not -1024
        if op in (5, 18, 4, 6):
            assert (Yk[0, :, :, 0, 0] & 1).any() and (kc[b][:, :, :, 0, 0] & 1).any()
        if c[1] == 6:
            assert not Yk[0, :, :, 0, 0].any() and not kc[b][:, :, :, 0, 0].any()
            want = {1: 0, 12: 0, 19: -1024}[op]
            assert (ey[0, :, :, 0, 0] == (want if op != 12 else 0)).all() and not ec[:, :, :, 0, 0].any()
        if c[1] == 7:
            assert (Yk[0, :, :, 0, 0] == 99).all() and (kc[b][:, :, :, 0, 0] == 35).all()
            assert (ey[0, :, :, 0, 0] == {1: 0, 12: 99, 19: -1024}[op]).all() and (ec[:, :, :, 0, 0] == (0 if op == 12 else 35)).all()


# ================================================================================================== refusals
def test_refusals_launch_nothing_and_touch_nothing(sources):
    S = 28
    st, (Y8, C8, q8) = stage(S), sources[S]
    Hy, Wy = AR.grid_of(S)
    boxes = [(2, 4, 2 * S, 2 * S), (0, 0, S, S), (6, 8, S // 2, S // 2)]
    base = params_of(boxes, ops=[[("Brightness", 0.27, None), ("Rotate90", 1.0, None)]] * 3)
    inp = Inputs(Y8, C8, q8, np.arange(3), boxes)
    pinp = Inputs(Y8, C8, q8, np.arange(3), boxes, packed=True)
    small = Inputs(Y8, C8[:, :, :20, :24].copy(), q8, np.arange(3), boxes)              # a chroma grid the boxes do not fit

    def mutated(**fields):
        arr, _ = st.pack(base)
        for k, v in fields.items():
            if k in ("op0", "op1"):
                arr[1].op[int(k[2])] = v
            else:
                setattr(arr[1], k, v)
        return arr

    good, _ = st.pack(base)
    cases = [("workspace one byte short", EWORKSPACE, Prepared(st, inp, good, 2, short=1)),
             ("y_off without c_off", EINVAL, Prepared(st, pinp, good, 2, drop_coff=True)),
             ("odd crop_i", EINVAL, Prepared(st, inp, mutated(crop_i=1), 2)),
             ("odd crop_j", EINVAL, Prepared(st, inp, mutated(crop_j=3), 2)),
             ("negative crop_i", EINVAL, Prepared(st, inp, mutated(crop_i=-2), 2)),
             ("negative crop_j", EINVAL, Prepared(st, inp, mutated(crop_j=-2), 2)),
             ("box below the grid", EINVAL, Prepared(st, inp, mutated(crop_i=Hy - S + 2), 2)),
             ("box right of the grid", EINVAL, Prepared(st, inp, mutated(crop_j=Wy - S + 2), 2)),
             ("box outside the chroma grid", EINVAL, Prepared(st, small, good, 2)),
             ("packed: box below the grid", EINVAL, Prepared(st, pinp, mutated(crop_i=Hy - S + 2), 2)),
             ("crop side 30", EINVAL, Prepared(st, inp, mutated(crop_h=30, crop_w=30), 2)),
             ("crop_h != crop_w", EINVAL, Prepared(st, inp, mutated(crop_h=S // 2), 2)),
             ("op id 20", EINVAL, Prepared(st, inp, mutated(op0=20), 2)),
             ("op id -1 in slot 1", EINVAL, Prepared(st, inp, mutated(op1=-1), 2)),
             ("nops 3", EINVAL, Prepared(st, inp, good, 3)),
             ("size 30", EINVAL, Prepared(st, inp, good, 2, size=30)),
             ("out_dtype 3", EINVAL, Prepared(st, inp, good, 2, odt=3)),
             ("B = 0", EINVAL, Prepared(st, inp, good, 2, B=0)),
             ("MidfreqAug without filters", EINVAL, Prepared(st, inp, mutated(op0=7), 2, filt=False)),
             ("Sharpness in slot 1 without filters", EINVAL, Prepared(st, inp, mutated(op1=15), 2, filt=False)),
             ("packed: Sharpness without filters", EINVAL, Prepared(st, pinp, mutated(op0=15), 2, filt=False))]
    torch.cuda.synchronize()
    rcs, names = KC.launched(lambda: [p.fire() for _n, _c, p in cases])
    assert not names, f"refused calls dispatched {names}"
    for (name, code, p), rc in zip(cases, rcs):
        assert rc == code, f"{name}: returned {rc}, expected {code}"
        assert p.untouched(), f"{name}: a guarded buffer was written"
    # the control: the same arguments without a mutation run, with and without filters where no op needs them
    for kw in (dict(), dict(filt=False)):
        for i in (inp, pinp):
            p = Prepared(st, i, good, 2, **kw)
            assert p.fire() == 0
            torch.cuda.synchronize()
            assert not p.untouched()
