"""The batched DFT-plane kernels behind the transform classes: RandAugment_dct(dft_kernel=True) and TrainTransform_DCT(dft_ops=True)
against the numpy oracles (oracle/dct_np.py for the kernel ops, oracle/dft_np.py for Rotate / ShearX / ShearY -- whose parity with
torchvision stays UNPINNED, see there).

Bounds as in tests/test_transform_classes.py::test_dft_plane_rotate_and_shear_vs_oracle, which holds the tensor path to them: the
matrix products are summed in another order than the oracle's, so results on a rounding tie move by one: |d| <= 1 on less than 2e-3
of a plane after one DFT-plane op and 2e-2 after two (the second one spreads every 1-LSB difference of its input over its whole
output).  Quarter turns are index work and exact."""
import numpy as np
import pytest
import torch

from oracle import dct_np as O
from oracle import dft_np as D
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import detfill

pytestmark = pytest.mark.gpu
DEV = "cuda"
R2 = 2 ** 0.5


def coeffs(B, H, W, seed):
    return (detfill.integers((B, 1, H, W, 8, 8), seed, -1024, 1016), detfill.integers((B, 2, H // 2, W // 2, 8, 8), seed + 1, -1024, 1016))


def dev(a):
    return torch.from_numpy(a).to(DEV)


def chain_ref(ry, rc, ops):
    """the reference's op loop (custom_transforms.py:1106-1123) on clamped int16 planes; returns the planes and the DFT-plane op count"""
    n = 0
    for name, mag, aux in ops:
        if name in CT.DFT_OPS:
            ry, rc = D.apply_dft_op(ry, rc, name, mag, pad=R2)
            ry, rc = np.clip(ry, O.CMIN, O.CMAX), np.clip(rc, O.CMIN, O.CMAX)
            n += 1
        else:
            ry, rc = O.apply_op(ry, rc, name, mag, aux)
    return ry, rc, n


def close(got, ref, ndft, where):
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    bound = 2e-3 if ndft < 2 else 2e-2
    print(where, "max", int(d.max()), "share", float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() < bound, (where, int(d.max()), float((d > 0).mean()))


META = CT.magnitude_table(11, (28, 28))
RA_CASES = [[("Rotate", 9.0, None), ("Brightness", 0.27, None)],
            [("Contrast", -0.27, None), ("ShearX", float(META["ShearX"][0][3]), None)],
            [("ShearY", -float(META["ShearY"][0][3]), None), ("Rotate", -100.0, None)],
            [("Rotate", 90.0, None), ("TranslateX", float(META["TranslateX"][0][3]), None)]]


@pytest.mark.parametrize("ops", RA_CASES, ids=["rotate-first", "shearx-last", "sheary-rotate", "quarter-turn"])
def test_randaugment_with_the_kernels_vs_oracle(ops):
    """The four op lists of test_dft_plane_rotate_and_shear_vs_oracle through RandAugment_dct(dft_kernel=True).  (Without a clamp
    after the DFT-plane op, as the tensor path: RandAugment_dct hands the next kernel pass what rotate_block / shear_block return.)"""
    Y, C = coeffs(2, 28, 28, 77)
    ra = CT.RandAugment_dct(num_ops=2, magnitude=3, dft_kernel=True)
    oy, oc = ra((dev(Y), dev(C)), ops=ops)
    assert oy.dtype == torch.int16 and oc.shape == (2, 2, 14, 14, 8, 8)
    for b in range(2):
        ry, rc = np.clip(Y[b], -1024, 1016), np.clip(C[b], -1024, 1016)
        for name, mag, aux in ops:
            if name in CT.DFT_OPS:
                ry, rc = D.apply_dft_op(ry, rc, name, mag, pad=R2)
            else:
                ry, rc = O.apply_op(ry, rc, name, mag, aux)
        ndft = sum(o[0] in CT.DFT_OPS for o in ops)
        if ops[0] == ("Rotate", 90.0, None):          # exact index work
            assert np.array_equal(oy[b].cpu().numpy(), ry) and np.array_equal(oc[b].cpu().numpy(), rc)
        else:
            close(oy[b].cpu().numpy(), ry, ndft, (ops, b, "Y"))
            close(oc[b].cpu().numpy(), rc, ndft, (ops, b, "C"))


def test_randaugment_quarter_turns_and_sampling_with_the_kernels():
    Y, C = coeffs(2, 28, 28, 77)
    oy, oc = CT.RandAugment_dct(num_ops=1, pad=False, dft_kernel=True)((dev(Y), dev(C)), ops=[("Rotate", -90.0, None)])
    assert np.array_equal(oy[1].cpu().numpy(), O.rotate90(np.clip(Y[1], -1024, 1016), -1))
    assert np.array_equal(oc[1].cpu().numpy(), O.rotate90(np.clip(C[1], -1024, 1016), -1))
    # per-sample draws: some samples carry a DFT-plane op in a pass, some do not; luma only works too
    torch.manual_seed(5)
    ra = CT.RandAugment_dct(num_ops=2, magnitude=5, ops_list=["Rotate", "ShearX", "ShearY", "Color"], dft_kernel=True)
    sy, sc = ra((dev(Y), dev(C)))
    assert sy.dtype == torch.int16 and sy.shape == (2, 1, 28, 28, 8, 8) and sc.dtype == torch.int16
    ly = ra(dev(Y), ops=[("Rotate", 9.0, None)])
    ky, _ = ra((dev(Y), dev(C)), ops=[("Rotate", 9.0, None)])
    assert torch.equal(ly, ky)
    # the same explicit op through both paths: the tensor path's result up to rounding ties
    ty, tc = CT.RandAugment_dct(num_ops=1)((dev(Y), dev(C)), ops=[("Rotate", 9.0, None)])
    ky, kc = CT.RandAugment_dct(num_ops=1, dft_kernel=True)((dev(Y), dev(C)), ops=[("Rotate", 9.0, None)])
    close(ky.cpu().numpy(), ty.cpu().numpy(), 1, "kernel vs tensor path Y")
    close(kc.cpu().numpy(), tc.cpu().numpy(), 1, "kernel vs tensor path C")


# ---- the fused transform: B = 4 on a 64-block source; a DFT-plane op first, last, between kernel ops, and two of them.
# Crop sides of 28 blocks: the resize stage is then the identity and exact.  A resize by 2 or 1/2 rounds a quarter of its DC
# coefficients on exact .5 ties, which fp32 decides either way (tests/test_augment.py excludes them for that reason); a DFT-plane op
# behind it spreads each such LSB over its whole output, which says nothing about the op.  The resizing boxes run in
# test_fused_transform_without_dft_ops_keeps_its_bits.
B = 4
BOXES = [(10, 4, 28, 28), (0, 36, 28, 28), (36, 20, 28, 28), (30, 2, 28, 28)]
FLIPS = [False, True, True, False]
OPSS = [[("Rotate", 9.0, None), ("Brightness", 0.27, None)],
        [("Contrast", -0.27, None), ("ShearX", float(META["ShearX"][0][3]), None)],
        [("TranslateX", float(META["TranslateX"][0][3]), None), ("ShearY", -float(META["ShearY"][0][3]), None), ("Rotate90", 1.0, None)],
        [("Rotate", -100.0, None), ("Color", -0.27, None), ("ShearX", -float(META["ShearX"][0][3]), None)]]
_FUSED_REF = {}


def fused_ref():
    """oracle crop / resize / flip, entry clamp, the op loop with the per-op clamp: the int16 stage in front of ToRange, once."""
    if not _FUSED_REF:
        Y, C = coeffs(B, 64, 64, 51)
        for b in range(B):
            i, j, h, w = BOXES[b]
            ry = O.resize(O.crop(Y[b], i, j, h, w), 28)
            rc = O.resize(O.crop(C[b], i // 2, j // 2, h // 2, w // 2), 14)
            if FLIPS[b]:
                ry, rc = O.flip(ry), O.flip(rc)
            ry, rc = np.clip(ry, O.CMIN, O.CMAX), np.clip(rc, O.CMIN, O.CMAX)
            _FUSED_REF[b] = chain_ref(ry, rc, OPSS[b])
    return _FUSED_REF


@pytest.mark.parametrize("odt", [torch.float32, torch.float16, torch.int16], ids=["f32", "f16", "i16"])
def test_fused_transform_with_dft_ops_vs_oracle(odt):
    Y, C = coeffs(B, 64, 64, 51)
    t = CT.TrainTransform_DCT(size=28, num_ops=3, ops_list=list(CT.REFERENCE_DEFAULT_OPS) + ["Rotate90"], out_dtype=odt, dft_ops=True)
    params = [dict(box=BOXES[b], flip=FLIPS[b], ops=OPSS[b]) for b in range(B)]
    fy, fc = t(dev(Y), dev(C), t._unit_quant(B, DEV), params=params)
    assert fy.dtype == odt and fc.dtype == odt and tuple(fy.shape) == (B, 1, 28, 28, 8, 8) and tuple(fc.shape) == (B, 2, 14, 14, 8, 8)
    ref = fused_ref()
    for b in range(B):
        ry, rc, ndft = ref[b]
        for got, r, nm in ((fy[b], ry, "Y"), (fc[b], rc, "C")):
            got = got.float().cpu().numpy()
            if odt != torch.int16:
                # ToRange maps one LSB of the int16 stage to 2 / 2040; fp16 rounds the result by at most a quarter of that on [-1, 1]
                lsb = (got.astype(np.float64) + 1.0) / 2.0 * 2040.0 - 1024.0
                assert np.abs(lsb - np.rint(lsb)).max() < (0.26 if odt == torch.float16 else 1e-3)
                got = np.rint(lsb)
            assert got.min() >= O.CMIN and got.max() <= O.CMAX
            close(got, r, ndft, (str(odt), b, nm))


def test_fused_transform_without_dft_ops_keeps_its_bits():
    Y, C = coeffs(B, 64, 64, 51)
    opss = [[("Contrast", 0.27, None), ("TranslateY", float(META["TranslateY"][0][3]), None)],
            [("Cutout", float(META["Cutout"][0][3]), (4, 20)), ("AutoContrast", 0.0, None)],
            [("MidfreqAug", -0.27, None), ("ChromaDrop", 0.0, True)], [("Rotate90", -1.0, None), ("AutoSaturation", 0.0, None)]]
    boxes = [(0, 0, 56, 56), (10, 4, 28, 28), (30, 40, 14, 14), (8, 8, 56, 56)]
    params = [dict(box=boxes[b], flip=bool(b & 1), ops=opss[b]) for b in range(B)]
    for odt in (torch.float32, torch.float16):
        a = CT.TrainTransform_DCT(size=28, out_dtype=odt)
        b_ = CT.TrainTransform_DCT(size=28, out_dtype=odt, dft_ops=True)
        ay, ac = a(dev(Y), dev(C), a._unit_quant(B, DEV), params=params)
        by, bc = b_(dev(Y), dev(C), b_._unit_quant(B, DEV), params=params)
        assert torch.equal(ay, by) and torch.equal(ac, bc)
    # explicit DFT-plane params without the opt-in are refused, like the constructor refuses the names
    plain = CT.TrainTransform_DCT(size=28)
    with pytest.raises(NotImplementedError):
        plain(dev(Y), dev(C), plain._unit_quant(B, DEV), params=[dict(box=boxes[1], flip=False, ops=[("Rotate", 9.0, None)])] * B)
    # sampled parameters with the reference's default list run end to end
    torch.manual_seed(2)
    s = CT.TrainTransform_DCT(size=28, ops_list=CT.REFERENCE_DEFAULT_OPS, dft_ops=True)
    sy, sc = s(dev(Y), dev(C), s._unit_quant(B, DEV))
    assert sy.dtype == torch.float32 and float(sy.abs().max()) <= 1.0 and bool(torch.isfinite(sc).all())
