"""The batched DFT-plane kernels (csrc/dft_ops.hip) at the C ABI (include/rgbnm.h: rgbnm_dct_dft_ops) against oracle/dft_np.py and
against the tensor path (dct_ops.rotate_block / shear_block on the device).  PARITY with torchvision stays UNPINNED, as the oracle
says; the contract here is the tensor path's result up to rounding ties.

Every run works in place on guarded Y / C buffers (kernel_check.guarded with the int16 canary in the margins) and on a guarded
workspace of exactly rgbnm_dct_dft_workspace bytes.  Inputs are detfill.integers(-1024, 1016).

Bounds.  Quarter turns and the zero shear resample with the identity map: the result is an integer before the final rounding and the
fp32 error of the round trip is far below 0.5, so the kernels must give the oracle's bits.  For the other angles the products are
summed in another order than the oracle's and the tensor path's, which moves results that lie on a rounding tie: max |d| <= 1 and at
most max(2, 2e-3 n) differing elements per plane of n elements (2e-3: the bound tests/test_transform_classes.py holds the tensor
path to against the same oracle; the tensor path itself differs from the oracle in at most 4.7e-4 of a plane on these cases)."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_check as KC
from oracle import dft_np as D
from rgb_no_more_amd import detfill
from rgb_no_more_amd import dct_ops as DO
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
R2 = 2 ** 0.5
CASES = [(2, False), (4, R2), (10, False), (28, R2), (32, R2)]
IDS = ["S2", "S4pad", "S10", "S28pad", "S32pad"]
EXACT_OPS = [("Rotate", 0.0), ("Rotate", 90.0), ("Rotate", -90.0), ("Rotate", 180.0), ("Rotate", 270.0), ("ShearX", 0.0)]
TIE_OPS = [("Rotate", 9.0), ("Rotate", 30.0), ("Rotate", -100.0), ("ShearX", 5.1), ("ShearY", -17.0)]


def plan(name, mag):
    if name == "Rotate":
        return DO.rotate_plan(mag)
    return DO.shear_plan(deg_x=mag) if name == "ShearX" else DO.shear_plan(deg_y=mag)


def inputs(B, S, seed):
    return (detfill.integers((B, 1, S, S, 8, 8), seed, -1024, 1016), detfill.integers((B, 2, S // 2, S // 2, 8, 8), seed + 1, -1024, 1016))


_ORACLE = {}


def oracle(S, pad, seed, b, name, mag):
    """oracle.dft_np.apply_dft_op of sample b of inputs(., S, seed): computed once per (case, op), never modified."""
    key = (S, pad, seed, b, name, mag)
    if key not in _ORACLE:
        Y, Cc = inputs(b + 1, S, seed)
        ry, rc = D.apply_dft_op(Y[b], Cc[b], name, mag, pad=pad)
        ry.setflags(write=False)
        rc.setflags(write=False)
        _ORACLE[key] = (ry, rc)
    return _ORACLE[key]


class Call:
    """One rgbnm_dct_dft_ops call on guarded buffers.  ops: {sample: (name, magnitude)}."""

    def __init__(self, Y, Cc, S, pad, ops, clamp=0, chroma=True):
        self.B, self.S = Y.shape[0], S
        self.Hy, self.Hc = DO.padded_blocks(S, pad), DO.padded_blocks(S // 2, pad)
        self.gy = KC.guarded(Y.size, None, torch.int16, device=DEV).fill_(torch.from_numpy(Y.reshape(-1)).to(DEV))
        self.gc = KC.guarded(Cc.size, None, torch.int16, device=DEV).fill_(torch.from_numpy(Cc.reshape(-1)).to(DEV)) if chroma else None
        self.Y0, self.C0 = Y, Cc
        mats, self.jobs = [], (L.DftJob * max(len(ops), 1))()
        for n, (b, (name, mag)) in enumerate(ops.items()):
            rot, mat = plan(name, mag)
            if mat not in mats:
                mats.append(mat)
            self.jobs[n].sample, self.jobs[n].rot90s = b, rot
            self.jobs[n].map_y = self.jobs[n].map_c = mats.index(mat)
        if not mats:
            mats.append(DO.shear_plan()[1])
        self.njobs, self.nmaps, self.clamp = len(ops), len(mats), clamp
        self.conv = [torch.view_as_real(DO.generate_conversion_matrix_dft(8, h, DEV)).contiguous() for h in (self.Hy, self.Hc)]
        self.maps = [torch.stack([DO.dft_gather_map(m, 8 * h, DEV) for m in mats]).contiguous() for h in (self.Hy, self.Hc)]
        self.ws_bytes = L.lib().rgbnm_dct_dft_workspace(max(self.njobs, 1), self.Hy, self.Hc)
        assert self.ws_bytes == max(self.njobs, 1) * 16 * ((8 * self.Hy) ** 2 + 2 * (8 * self.Hc) ** 2)
        self.ws = KC.guarded(self.ws_bytes // 4, None, torch.float32, device=DEV)

    def jobs_dev(self):
        return torch.from_numpy(np.frombuffer(bytes(self.jobs), dtype=np.uint8).copy()).to(DEV)

    def run(self, **over):
        a = dict(Y=self.gy.t.data_ptr(), C=L.ptr(self.gc.t) if self.gc is not None else None, B=self.B, S=self.S, Hy=self.Hy,
                 Hc=self.Hc, jd=self.jobs_dev(), jh=C.cast(self.jobs, C.c_void_p), njobs=self.njobs, nmaps=self.nmaps,
                 clamp=self.clamp, ws_bytes=self.ws_bytes)
        a.update(over)
        rc = L.lib().rgbnm_dct_dft_ops(a["Y"], a["C"], a["B"], a["S"], a["Hy"], a["Hc"], L.ptr(a["jd"]), a["jh"], a["njobs"],
                                       self.conv[0].data_ptr(), self.conv[1].data_ptr(), self.maps[0].data_ptr(),
                                       self.maps[1].data_ptr(), a["nmaps"], a["clamp"], self.ws.t.data_ptr(), a["ws_bytes"], L.stream())
        torch.cuda.synchronize()
        return rc

    def out(self, where=""):
        """(Y, C) as numpy after checking every margin."""
        self.gy.check(where + " Y", written=False)
        self.ws.check(where + " workspace", written=False)
        y = self.gy.t.cpu().numpy().reshape(self.Y0.shape)
        if self.gc is None:
            return y, None
        self.gc.check(where + " C", written=False)
        return y, self.gc.t.cpu().numpy().reshape(self.C0.shape)

    def untouched(self, where):
        y, c = self.out(where)
        assert np.array_equal(y, self.Y0), where
        assert c is None or np.array_equal(c, self.C0), where


def ties(got, ref, where):
    """max |d| <= 1 and at most max(2, 2e-3 n) differing elements, per plane."""
    worst = 0.0
    for p in range(got.shape[0]):
        d = np.abs(got[p].astype(np.int32) - ref[p].astype(np.int32))
        n, k = d.size, int((d > 0).sum())
        worst = max(worst, k / n)
        assert d.max() <= 1 and k <= max(2, 2e-3 * n), (where, p, int(d.max()), k, n)
    return worst


@pytest.mark.parametrize("S,pad", CASES, ids=IDS)
def test_identity_map_cases_are_bit_exact(S, pad):
    """Quarter turns and the zero shear: every index fold (pad, quarter turn of the padded grid, shifts, crop) against the oracle."""
    B, seed = len(EXACT_OPS), 100 + S
    Y, Cc = inputs(B, S, seed)
    call = Call(Y, Cc, S, pad, dict(enumerate(EXACT_OPS)))
    assert call.run() == 0
    y, c = call.out(f"exact S={S}")
    for b, (name, mag) in enumerate(EXACT_OPS):
        ry, rc = oracle(S, pad, seed, b, name, mag)
        assert np.array_equal(y[b], ry), (S, pad, name, mag, "Y", int(np.abs(y[b].astype(int) - ry).max()))
        assert np.array_equal(c[b], rc), (S, pad, name, mag, "C", int(np.abs(c[b].astype(int) - rc).max()))


@pytest.mark.parametrize("S,pad", CASES, ids=IDS)
def test_against_the_tensor_path_and_the_oracle(S, pad):
    B, seed = len(TIE_OPS), 200 + S
    Y, Cc = inputs(B, S, seed)
    call = Call(Y, Cc, S, pad, dict(enumerate(TIE_OPS)))
    assert call.run() == 0
    y, c = call.out(f"ties S={S}")
    clamped = Call(Y, Cc, S, pad, dict(enumerate(TIE_OPS)), clamp=1)
    assert clamped.run() == 0
    yk, ck = clamped.out(f"clamp S={S}")
    peak = 0
    for b, (name, mag) in enumerate(TIE_OPS):
        ry, rc = oracle(S, pad, seed, b, name, mag)
        if name == "Rotate":
            f = lambda t: DO.rotate_block(t, degrees=mag, pad=pad)                 # noqa: E731
        else:
            f = lambda t: DO.shear_block(t, pad=pad, **{"deg_x" if name == "ShearX" else "deg_y": mag})      # noqa: E731
        ty, tc = f(torch.from_numpy(Y[b]).to(DEV)).cpu().numpy(), f(torch.from_numpy(Cc[b]).to(DEV)).cpu().numpy()
        w = [ties(y[b], ry, (S, name, mag, "Y oracle")), ties(c[b], rc, (S, name, mag, "C oracle")),
             ties(y[b], ty, (S, name, mag, "Y tensor")), ties(c[b], tc, (S, name, mag, "C tensor")),
             ties(yk[b], np.clip(ry, -1024, 1016), (S, name, mag, "Y clamp")), ties(ck[b], np.clip(rc, -1024, 1016), (S, name, mag, "C clamp"))]
        print(f"S={S} {name} {mag}: differing share vs oracle Y {w[0]:.2e} C {w[1]:.2e}, vs tensor path Y {w[2]:.2e} C {w[3]:.2e}, "
              f"clamped Y {w[4]:.2e} C {w[5]:.2e}")
        assert yk[b].min() >= -1024 and yk[b].max() <= 1016 and ck[b].min() >= -1024 and ck[b].max() <= 1016
        peak = max(peak, int(np.abs(ry).max()))
    assert peak > 1016, "these inputs leave the coefficient range: the clamp is exercised"


@pytest.mark.parametrize("S,pad", [(4, R2), (28, R2)], ids=["S4pad", "S28pad"])
def test_jobs_are_independent_of_the_batch_and_of_the_run(S, pad):
    """Five jobs in a batch of 7: each listed sample has the bits of the same sample run alone, the two others are untouched, a
    second run gives the same bits, and luma comes out the same without chroma (C == NULL)."""
    B, seed = 7, 300 + S
    Y, Cc = inputs(B, S, seed)
    ops = {5: ("Rotate", 30.0), 0: ("ShearX", 5.1), 3: ("Rotate", -100.0), 6: ("ShearY", -17.0), 2: ("Rotate", 9.0)}
    call = Call(Y, Cc, S, pad, ops, clamp=1)
    assert call.run() == 0
    y, c = call.out("batch")
    again = Call(Y, Cc, S, pad, ops, clamp=1)
    assert again.run() == 0
    y2, c2 = again.out("batch, second run")
    assert np.array_equal(y, y2) and np.array_equal(c, c2)
    for b in (1, 4):
        assert np.array_equal(y[b], Y[b]) and np.array_equal(c[b], Cc[b]), f"sample {b} is not listed"
    for b, op in ops.items():
        alone = Call(Y[b:b + 1], Cc[b:b + 1], S, pad, {0: op}, clamp=1)
        assert alone.run() == 0
        ya, ca = alone.out(f"alone {b}")
        assert np.array_equal(ya[0], y[b]) and np.array_equal(ca[0], c[b]), (b, op)
        assert not np.array_equal(y[b], Y[b])
    luma = Call(Y, Cc, S, pad, ops, clamp=1, chroma=False)
    assert luma.run() == 0
    yl, _ = luma.out("C == NULL")
    assert np.array_equal(yl, y)


def test_refusals_leave_the_outputs_unwritten():
    S, pad = 4, R2
    Y, Cc = inputs(3, S, 400)
    ops = {0: ("Rotate", 9.0), 2: ("ShearX", 5.1)}

    def refused(where, edit=None, **over):
        call = Call(Y, Cc, S, pad, ops)
        if edit is not None:
            edit(call.jobs)
        assert call.run(**over) == EINVAL, where
        call.untouched(where)

    refused("odd S", S=3)
    refused("S = 0", S=0)
    refused("S = 34", S=34, Hy=48, Hc=24)
    refused("Hp_y < Hb", Hy=3)
    refused("Hp_c < Hb", Hc=1)
    refused("Hp_y > 48", Hy=49)
    refused("Hp_c > 48", Hc=49)
    refused("njobs < 0", njobs=-1)
    refused("jobs_host missing", jh=None)
    refused("jobs_dev missing", jd=None)
    refused("sample = B", lambda j: setattr(j[1], "sample", 3))
    refused("sample < 0", lambda j: setattr(j[0], "sample", -1))
    refused("sample twice", lambda j: setattr(j[1], "sample", 0))
    refused("rot90s = 4", lambda j: setattr(j[0], "rot90s", 4))
    refused("rot90s < 0", lambda j: setattr(j[1], "rot90s", -1))
    refused("map_y = nmaps", lambda j: setattr(j[0], "map_y", 2))
    refused("map_c < 0", lambda j: setattr(j[1], "map_c", -1))
    refused("clamp = 2", clamp=2)
    refused("clamp < 0", clamp=-1)
    call = Call(Y, Cc, S, pad, ops)
    assert call.run(ws_bytes=call.ws_bytes - 1) == EINVAL
    call.untouched("short workspace")
    # njobs == 0: nothing to do, nothing launched
    empty = Call(Y, Cc, S, pad, {})
    (_, names) = KC.launched(lambda: empty.run())
    assert empty.run() == 0 and not KC.ran(names, "dftops")
    empty.untouched("njobs = 0")
    # and the call that is not refused does launch the four stages
    call = Call(Y, Cc, S, pad, ops)
    rc, names = KC.launched(lambda: call.run())
    assert rc == 0 and sum("dftops" in n for n in names) == 4, names
