"""rgbnm_dct_augment_chain at the C ABI: RandAugment chains of more than two operations in kernel 2's one launch, the fp16 output,
the same bits as rgbnm_dct_augment_ex / _packed where those run, and the refusals.

Reference, as in tests/test_augment_edges.py: augment_ref.expected_ops on kernel 1's OWN int16 output, read back through the new
entry with out_code 2 and nops 0; ToRange by the oracle in fp32; fp16 = torch's .half() of that.  Every comparison is bit exact
and every output lies in a guarded buffer (kernel_check)."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_ref as AR
import kernel_check as KC
import test_augment_edges as TE
from oracle import dct_np as O
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EWORKSPACE = -1, -3
OUT = {"i16": (torch.int16, 2), "f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "f16": (torch.float16, 3)}
_BITS = {2: torch.int16, 4: torch.int32}


# ================================================================================================== harness
def pack_ops(st, params):
    """TrainTransform_DCT.pack_chain; an op ("raw", id, fmag, iarg0, iarg1, iarg2) is written into its record as it is."""
    named = [dict(p, ops=[("Identity", 0.0, None) if o[0] == "raw" else o for o in p["ops"]]) for p in params]
    arr, ops, nops = st.t.pack_chain(named)
    for b, p in enumerate(params):
        for s, o in enumerate(p["ops"]):
            if o[0] == "raw":
                ops[b, s] = tuple(o[1:])
    return arr, ops, nops


class Call:
    """One call of rgbnm_dct_augment_chain with guarded outputs and workspace.  ops: AUG_OP_DTYPE (B, nops) or None (ops from the
    parameters); drop: arguments passed as NULL although they exist ("ops_dev", "ops_host", "c_off")."""

    def __init__(self, st, inp, arr, nops, ops=None, variant=0, entry=1, out="i16", short=0, filt=True, B=None, size=None,
                 odt=None, drop=()):
        S, nB = st.S, inp.B
        dt, code = OUT[out]
        ny, nc = nB * S * S * 64, nB * 2 * (S // 2) ** 2 * 64
        mk = (lambda n: AR.guarded_i16(n)) if out == "i16" else (lambda n: KC.guarded(n, None, dt))
        self.gy, self.gc = mk(ny), mk(nc)
        wsb = L.lib().rgbnm_dct_augment_workspace_ex(nB, S)
        self.gw = AR.guarded_i16(wsb // 2)
        self.pdev = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(DEV)
        odev = ohost = None
        if ops is not None:
            # backing of at least one record, so that nops = 0 still hands over two non-NULL pointers
            self.ohost = np.zeros(max(ops.size, 1), dtype=CT.AUG_OP_DTYPE)
            self.ohost[:ops.size] = ops.reshape(-1)
            self.odev = torch.from_numpy(self.ohost.view(np.uint8).copy()).to(DEV)
            odev, ohost = self.odev.data_ptr(), self.ohost.ctypes.data
        f = st.t.bank.device_tensor(DEV) if filt else None
        Yd, Cd, yo, co = inp.variants[variant]
        self.keep = (arr, f, Yd, Cd, yo, co, inp.qd)
        self.args = (Yd.data_ptr(), L.ptr(Cd), L.ptr(yo), None if "c_off" in drop else L.ptr(co), inp.qd.data_ptr(),
                     self.pdev.data_ptr(), C.cast(arr, C.c_void_p), None if "ops_dev" in drop else odev,
                     None if "ops_host" in drop else ohost, st.A.data_ptr(), L.ptr(f), self.gy.t.data_ptr(), self.gc.t.data_ptr(),
                     code if odt is None else odt, S if size is None else size, nB if B is None else B, inp.Hy, inp.Wy, inp.Hc,
                     inp.Wc, entry, nops, self.gw.t.data_ptr(), wsb - short, L.stream())

    def fire(self):
        return L.lib().rgbnm_dct_augment_chain(*self.args)

    def bits(self):
        """(outY, outC) as integer tensors on the host: the stored bits."""
        return tuple(g.t.view(_BITS[g.esz]).cpu() for g in (self.gy, self.gc))

    def untouched(self):
        return all(bool((g.raw == g.canary).all()) for g in (self.gy, self.gc, self.gw))


def run(st, inp, arr, nops, where, written=True, ws_written=True, **kw):
    """Code 0, guards intact, every output element written -> the bits of (outY [B, ...], outC [B, ...]).  written / ws_written
    False: the outputs / the int16 workspace may hold the canary's value as data."""
    c = Call(st, inp, arr, nops, **kw)
    rc = c.fire()
    torch.cuda.synchronize()
    assert rc == 0, f"{where}: rgbnm error {rc}"
    c.gy.check(f"{where} outY", written=written)
    c.gc.check(f"{where} outC", written=written)
    c.gw.check(f"{where} workspace", written=written and ws_written)
    y, cc = c.bits()
    S = st.S
    return y.reshape(inp.B, 1, S, S, 8, 8), cc.reshape(inp.B, 2, S // 2, S // 2, 8, 8)


def want_bits(x, out):
    """int16 coefficients -> the bits the stage must store for output type `out`."""
    if out == "i16":
        return torch.from_numpy(np.ascontiguousarray(x))
    r = torch.from_numpy(O.to_range(x))
    if out == "f32":
        return r.view(torch.int32)
    return (r.bfloat16() if out == "bf16" else r.half()).view(torch.int16)


def scaled_sources(S):
    """Three source images on the batch grid of S whose de-quantised values leave [-1024, 1016] and wrap int16 (tables x 9)."""
    Hy, Wy = AR.grid_of(S)
    Y, Cc, q = TE.synth_grid(3, Hy, Wy, Hy // 2, Wy // 2, seed=70 + S)
    q = (q.astype(np.int32) * 9).astype(np.int16)
    Y[:, 0, 1::3, 2::5, 1, 1] = 12000
    Y[:, 0, ::4, 1::3, 3, 3] = -1024
    return Y, Cc, q


@pytest.fixture(scope="module")
def sources():
    return {S: scaled_sources(S) for S in (28, 32)}


def chains(S, nops):
    """One chain per image (sides 2 S, S, S / 2).  Slot 0 is an op that tests/test_augment_edges.py runs first on an unclamped
    image (a whole-image permutation, a partial zeroing, a rectangle); slots >= 2 hold the in-place permutations, the reductions,
    Solarize (LDS mask), both filter ops and Cutout.  Image 2 has fewer real ops than nops: its chain is padded with Identity."""
    c0 = [("Rotate90", -1.0, None), ("Posterize", 2.0, None), ("Rotate90", 1.0, None), ("AutoContrast", 0.0, None),
          ("Solarize", 100.5, None), ("MidfreqAug", 0.27, None), ("Cutout", 5.6, (10, 4)), ("TranslateX", -3.75, None)]
    c1 = [("ChromaDrop", 0.0, True), ("TranslateY", -3.75, None), ("Rotate90", -1.0, None), ("Equalize", 0.0, None),
          ("Sharpness", -0.27, None), ("AutoSaturation", 0.0, None), ("TranslateY", 3.75, None), ("Solarize", -163.6, None)]
    c2 = [("raw", 8, 0.0, 4, S - 1, 0), ("Contrast", 0.27, None), ("TranslateX", 3.75, None)]
    pick = {3: lambda c: c[:2] + c[7:8], 4: lambda c: c[:2] + c[4:6], 8: lambda c: c}[nops]
    return [pick(c0), pick(c1), c2[:min(3, nops - 1)]]


def batch(S, sources, packed):
    Y8, C8, q8 = sources[S]
    Hy, Wy = AR.grid_of(S)
    boxes = AR.boxes_for([2 * S, S, S // 2], Hy, Wy)
    return boxes, TE.Inputs(Y8, C8, q8, np.arange(3), boxes, packed=packed)


def outside(x):
    return bool((x > AR.CMAX).any() or (x < AR.CMIN).any())


# ================================================================================================== chains
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("S", [28, 32])
def test_chains_of_3_4_8_ops_every_output_code(S, packed, sources):
    st = TE.stage(S)
    boxes, inp = batch(S, sources, packed)
    filt = st.filters_np()
    for entry in (1, 2):
        base = TE.params_of(boxes, flips=[1, 0, 1])
        arr0, _ = st.pack(base)
        ky, kc = run(st, inp, arr0, 0, f"S{S} entry {entry} kernel 1", entry=entry, written=entry == 1)
        ky, kc = ky.numpy(), kc.numpy()
        if entry == 2:       # raw input, unclamped entry: the image leaves the range, the canary value does not occur in it
            assert outside(ky) and not (ky == AR.I16_CANARY).any() and not (kc == AR.I16_CANARY).any()
        for nops in (3, 4, 8):
            params = TE.params_of(boxes, flips=[1, 0, 1], ops=chains(S, nops))
            arr, ops, n = pack_ops(st, params)
            assert n == nops and ops.shape == (3, nops) and len(params[2]["ops"]) < nops
            exp = [AR.expected_ops(ky[b], kc[b], p["ops"], filters=filt) for b, p in enumerate(params)]
            for b in range(3):
                assert not outside(exp[b][0]) and not outside(exp[b][1])
            for out in (("i16", "f32", "bf16", "f16") if (entry, nops) == (1, 4) else ("i16",)):
                where = f"S{S} packed {packed} entry {entry} nops {nops} {out}"
                oy, oc = run(st, inp, arr, nops, where, ops=ops, entry=entry, out=out)
                for b, p in enumerate(params):
                    assert torch.equal(oy[b], want_bits(exp[b][0], out)), (where, b, p["ops"], "Y")
                    assert torch.equal(oc[b], want_bits(exp[b][1], out)), (where, b, p["ops"], "C")


def test_every_int16_value_to_f16():
    """One S = 28 image holding every int16 value (75 264 coefficients >= 65 536), unit tables, entry_clamp 2, no ops, identity
    crop: the f16 output is .half() of the fp32 ToRange of every value, the fp32 output is that ToRange itself."""
    S = 28
    st = TE.stage(S)
    vals = ((np.arange(AR.units(S) * 64, dtype=np.int64) * 40503 + 32768) % 65536 - 32768).astype(np.int16)   # 40503 is odd: a bijection per 65536
    assert np.unique(vals).size == 65536
    Y8 = vals[:S * S * 64].reshape(1, 1, S, S, 8, 8).copy()
    C8 = vals[S * S * 64:].reshape(1, 2, S // 2, S // 2, 8, 8).copy()
    q8 = np.ones((1, 3, 8, 8), np.int16)
    boxes = [(0, 0, S, S)]
    inp = TE.Inputs(Y8, C8, q8, np.arange(1), boxes)
    arr, _ = st.pack(TE.params_of(boxes, flips=[0]))
    for out in ("f32", "f16"):
        oy, oc = run(st, inp, arr, 0, f"every int16 -> {out}", entry=2, out=out, ws_written=False)      # the image holds 0x7FC5
        assert torch.equal(oy[0], want_bits(Y8[0], out)), out
        assert torch.equal(oc[0], want_bits(C8[0], out)), out
        assert torch.equal(oc.reshape(-1)[-8:], want_bits(C8, out).reshape(-1)[-8:])          # the chroma planes' tail


# ================================================================================================== same bits as the old entries
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("S", [28, 32])
def test_same_bits_as_the_existing_entries(S, packed, sources):
    st = TE.stage(S)
    boxes, inp = batch(S, sources, packed)
    two = [[("Brightness", 0.27, None), ("Rotate90", 1.0, None)], [("MidfreqAug", -0.27, None), ("Cutout", 1.8, (12, 26))],
           [("Equalize", 0.0, None), ("TranslateY", 3.75, None)]]
    params = TE.params_of(boxes, flips=[0, 1, 1], ops=two)
    arr, _ = st.pack(params)
    _, ops2, _ = pack_ops(st, params)
    other, _ = st.pack(TE.params_of(boxes, flips=[0, 1, 1], ops=[[("Invert", 0.0, None), ("Grayscale", 0.0, None)]] * 3))
    for nops in (0, 1, 2):
        for out in ("f32", "bf16", "i16"):
            where = f"S{S} packed {packed} nops {nops} {out}"
            old = TE.Prepared(st, inp, arr, nops, out=out)
            assert old.fire() == 0
            torch.cuda.synchronize()
            want = tuple(g.t.view(_BITS[g.esz]).cpu().reshape(-1) for g in (old.gy, old.gc))
            got = run(st, inp, arr, nops, where + " ops from params", out=out)
            assert torch.equal(got[0].reshape(-1), want[0]) and torch.equal(got[1].reshape(-1), want[1]), where
            # ops from an array: the op fields of the parameters are not read (they hold other ops here)
            got = run(st, inp, other, nops, where + " ops from array", out=out, ops=np.ascontiguousarray(ops2[:, :nops]))
            assert torch.equal(got[0].reshape(-1), want[0]) and torch.equal(got[1].reshape(-1), want[1]), where


# ================================================================================================== refusals
def test_refusals_launch_nothing_and_touch_nothing(sources):
    S = 28
    st = TE.stage(S)
    Y8, C8, q8 = sources[S]
    Hy, Wy = AR.grid_of(S)
    boxes, inp = batch(S, sources, False)
    _, pinp = batch(S, sources, True)
    small = TE.Inputs(Y8, C8[:, :, :20, :24].copy(), q8, np.arange(3), boxes)              # a chroma grid the boxes do not fit
    params8 = TE.params_of(boxes, ops=[[("Brightness", 0.27, None), ("Rotate90", 1.0, None)] * 4] * 3)
    params2 = TE.params_of(boxes, ops=[[("Brightness", 0.27, None), ("Rotate90", 1.0, None)]] * 3)
    good, ops8, _ = pack_ops(st, params8)
    good2, _ = st.pack(params2)

    def mutated(**fields):
        arr, _ = st.pack(params2)
        for k, v in fields.items():
            if k in ("op0", "op1"):
                arr[1].op[int(k[2])] = v
            else:
                setattr(arr[1], k, v)
        return arr

    def with_op(slot, op):
        o = ops8.copy()
        o["op"][1, slot] = op
        return o

    nine = np.zeros((3, 9), dtype=CT.AUG_OP_DTYPE)
    cases = [("nops 9", EINVAL, Call(st, inp, good, 9, ops=nine)),
             ("nops -1 with an ops array", EINVAL, Call(st, inp, good, -1, ops=ops8)),
             ("nops -1 without", EINVAL, Call(st, inp, good2, -1)),
             ("nops 3 without an ops array", EINVAL, Call(st, inp, good2, 3)),
             ("ops_host alone", EINVAL, Call(st, inp, good, 8, ops=ops8, drop=("ops_dev",))),
             ("ops_dev alone", EINVAL, Call(st, inp, good, 8, ops=ops8, drop=("ops_host",))),
             ("out_code 4", EINVAL, Call(st, inp, good, 8, ops=ops8, odt=4)),
             ("out_code -1", EINVAL, Call(st, inp, good2, 2, odt=-1)),
             ("op id 20 in slot 5", EINVAL, Call(st, inp, good, 8, ops=with_op(5, 20))),
             ("op id -1 in slot 2", EINVAL, Call(st, inp, good, 8, ops=with_op(2, -1))),
             ("op id 20 in the last slot, packed", EINVAL, Call(st, pinp, good, 8, ops=with_op(7, 20))),
             ("MidfreqAug in slot 3 without filters", EINVAL, Call(st, inp, good, 8, ops=with_op(3, 7), filt=False)),
             ("Sharpness in slot 7 without filters", EINVAL, Call(st, inp, good, 8, ops=with_op(7, 15), filt=False)),
             # what the existing entries refuse
             ("workspace one byte short", EWORKSPACE, Call(st, inp, good, 8, ops=ops8, short=1)),
             ("y_off without c_off", EINVAL, Call(st, pinp, good, 8, ops=ops8, drop=("c_off",))),
             ("odd crop_i", EINVAL, Call(st, inp, mutated(crop_i=1), 2)),
             ("odd crop_j", EINVAL, Call(st, inp, mutated(crop_j=3), 2)),
             ("negative crop_i", EINVAL, Call(st, inp, mutated(crop_i=-2), 2)),
             ("negative crop_j", EINVAL, Call(st, inp, mutated(crop_j=-2), 2)),
             ("box below the grid", EINVAL, Call(st, inp, mutated(crop_i=Hy - S + 2), 2)),
             ("box right of the grid", EINVAL, Call(st, inp, mutated(crop_j=Wy - S + 2), 2)),
             ("box outside the chroma grid", EINVAL, Call(st, small, good, 8, ops=ops8)),
             ("packed: box below the grid", EINVAL, Call(st, pinp, mutated(crop_i=Hy - S + 2), 2)),
             ("crop side 30", EINVAL, Call(st, inp, mutated(crop_h=30, crop_w=30), 2)),
             ("crop_h != crop_w", EINVAL, Call(st, inp, mutated(crop_h=S // 2), 2)),
             ("op id 20 in the parameters", EINVAL, Call(st, inp, mutated(op0=20), 2)),
             ("op id -1 in slot 1 of the parameters", EINVAL, Call(st, inp, mutated(op1=-1), 2)),
             ("size 30", EINVAL, Call(st, inp, good, 8, ops=ops8, size=30)),
             ("B = 0", EINVAL, Call(st, inp, good, 8, ops=ops8, B=0)),
             ("MidfreqAug in the parameters without filters", EINVAL, Call(st, inp, mutated(op0=7), 2, filt=False)),
             ("packed: Sharpness in the parameters without filters", EINVAL, Call(st, pinp, mutated(op1=15), 2, filt=False))]
    torch.cuda.synchronize()
    rcs, names = KC.launched(lambda: [c.fire() for _n, _c, c in cases])
    assert not names, f"refused calls dispatched {names}"
    for (name, code, c), rc in zip(cases, rcs):
        assert rc == code, f"{name}: returned {rc}, expected {code}"
        assert c.untouched(), f"{name}: a guarded buffer was written"
    # the control: the same arguments without a mutation run, with and without filters where no op needs them; an op id in the
    # parameters that the ops array overrides is not looked at
    for kw in (dict(), dict(filt=False)):
        for i in (inp, pinp):
            for c in (Call(st, i, good, 8, ops=ops8, out="f16", **kw), Call(st, i, good2, 2, out="f16", **kw),
                      Call(st, i, mutated(op0=20), 8, ops=ops8, **kw)):
                assert c.fire() == 0
                torch.cuda.synchronize()
                c.gy.check("control outY")
                c.gc.check("control outC")
