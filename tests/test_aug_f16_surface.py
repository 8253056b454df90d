"""The Python surface of the fp16 data stage and of RandAugment chains beyond two operations: the fused transform, ToRange,
RandAugment_dct, get_transform, rgbnm_mixup_any / RandomMixup_DCT on fp16 items, and one ViT step fed the fp16 augment output."""
import numpy as np
import pytest
import torch

import kernel_check as KC
import test_augment as TA
import rgb_no_more_amd as rg
from oracle import dct_np as O
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import detfill
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def dev(a):
    return torch.from_numpy(a).to(DEV)


def half_of(x):
    return torch.from_numpy(np.ascontiguousarray(x)).half()


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


# ================================================================================================== fused transform, ToRange
THREE = [[("Posterize", 2.0, None), ("Rotate90", 1.0, None), ("Cutout", 1.8, (12, 26))],
         [("Color", 0.27, None), ("TranslateX", -3.75, None), ("AutoContrast", 0.0, None)]]


def test_fused_transform_writes_fp16_for_three_ops_and_in_eval_mode():
    """Identity resize (crop side 28): the whole chain is integer work, so the oracle's fp32 output rounded by .half() is the bits."""
    Y, Cc, quant = TA.synth(2, 40, 48, seed=31)
    params = [dict(box=(2, 4, 28, 28), flip=True, ops=THREE[0]), dict(box=(10, 16, 28, 28), flip=False, ops=THREE[1])]
    t = CT.TrainTransform_DCT(out_dtype=torch.float16, num_ops=3)
    oy, oc = t(dev(Y), dev(Cc), dev(quant), params=params)
    ry, rc = TA.run_oracle(Y, Cc, quant, params)
    assert oy.shape == (2, 1, 28, 28, 8, 8) and oc.shape == (2, 2, 14, 14, 8, 8)
    assert same_bits(oy, half_of(ry)) and same_bits(oc, half_of(rc))
    # two ops and fp16: the ops come from the parameters
    p2 = [dict(p, ops=p["ops"][:2]) for p in params]
    oy, oc = CT.TrainTransform_DCT(out_dtype=torch.float16)(dev(Y), dev(Cc), dev(quant), params=p2)
    ry, rc = TA.run_oracle(Y, Cc, quant, p2)
    assert same_bits(oy, half_of(ry)) and same_bits(oc, half_of(rc))
    # three ops and fp32: the chain entry with the old output types
    oy, oc = CT.TrainTransform_DCT(num_ops=3)(dev(Y), dev(Cc), dev(quant), params=params)
    ry, rc = TA.run_oracle(Y, Cc, quant, params)
    assert np.array_equal(oy.cpu().numpy(), ry) and np.array_equal(oc.cpu().numpy(), rc)
    # eval: no flip, no ops
    pe = [dict(box=p["box"], flip=False, ops=[]) for p in params]
    ey, ec = CT.EvalTransform_DCT(out_dtype=torch.float16)(dev(Y), dev(Cc), dev(quant), params=pe)
    ry, rc = TA.run_oracle(Y, Cc, quant, pe)
    assert same_bits(ey, half_of(ry)) and same_bits(ec, half_of(rc))
    with pytest.raises(NotImplementedError, match="per-transform"):
        CT.TrainTransform_DCT(num_ops=CT.AUG_MAX_OPS + 1)
    assert CT.TrainTransform_DCT(num_ops=CT.AUG_MAX_OPS).num_ops == 8


def test_torange_float16_kernel_and_tensor_op_paths():
    Y = detfill.integers((2, 1, 28, 28, 8, 8), 11, -1024, 1016)
    Cc = detfill.integers((2, 2, 14, 14, 8, 8), 12, -1024, 1016)
    ty, tc = CT.ToRange(-1, 1, -1024, 1016, torch.float16)((dev(Y), dev(Cc)))
    assert same_bits(ty, half_of(O.to_range(Y))) and same_bits(tc, half_of(O.to_range(Cc)))      # fp32 ToRange, one rounding
    # a 20 x 20 grid is not the kernels': the reference's statements in fp16 (cast first)
    Ys = detfill.integers((1, 20, 20, 8, 8), 13, -1024, 1016)
    g = CT.ToRange(-1, 1, -1024, 1016, torch.float16)(dev(Ys))
    x = torch.from_numpy(Ys).to(torch.float16)
    x = (x - (-1024)) / (1016 - (-1024))
    x = -1 + (x * (1 - (-1)))
    assert g.shape == (1, 20, 20, 8, 8) and same_bits(g, x)


def test_get_transform_fp16_three_ops_fused_and_composed():
    Y, Cc, quant = TA.synth(3, 64, 64, seed=32)
    torch.manual_seed(5)
    t = rg.datasets.get_transform("imagenet_dct", "train", num_ops=3, ops_magnitude=3, dtype=torch.float16, fused=True)
    assert isinstance(t, CT.TrainTransform_DCT) and t.num_ops == 3 and t.out_dtype == torch.float16
    oy, oc = t(dev(Y), dev(Cc), dev(quant))
    assert oy.dtype == oc.dtype == torch.float16 and oy.shape == (3, 1, 28, 28, 8, 8) and oc.shape == (3, 2, 14, 14, 8, 8)
    assert float(oy.float().abs().max()) <= 1.0 and float(oc.float().abs().max()) <= 1.0
    # the sampler's route: sample_chain -> apply_packed(ops=...)
    packed, ops, nops = CT.FastParamSampler(t, seed=3).sample_chain(3, 64, 64)
    assert nops == 3 and ops.shape == (3, 3)
    sy, sc = CT.apply_packed(t, dev(Y), dev(Cc), dev(quant), packed, nops, ops=ops)
    assert sy.dtype == torch.float16 and float(sy.float().abs().max()) <= 1.0 and float(sc.float().abs().max()) <= 1.0
    # ... equals forward() on the same parameters spelled out as records
    t32 = CT.TrainTransform_DCT(num_ops=3, magnitude=3, ops_list=CT.DEFAULT_OPS)
    t32.bank = t.bank
    f32y, f32c = CT.apply_packed(t32, dev(Y), dev(Cc), dev(quant), packed, nops, ops=ops)
    assert same_bits(sy, f32y.half()) and same_bits(sc, f32c.half())
    # the composed form (de-quantised coefficients in): the fused transform's bits on the same explicit parameters, then sampled
    Yd = detfill.integers((2, 1, 64, 64, 8, 8), 51, -1024, 1016)
    Cd = detfill.integers((2, 2, 32, 32, 8, 8), 52, -1024, 1016)
    boxes, flips = [(0, 0, 56, 56), (30, 40, 14, 14)], [True, False]
    fused = CT.TrainTransform_DCT(out_dtype=torch.float16, num_ops=3)
    fy, fc = fused(dev(Yd), dev(Cd), fused._unit_quant(2, DEV),
                   params=[dict(box=boxes[b], flip=flips[b], ops=THREE[b]) for b in range(2)])
    c = rg.datasets.get_transform("imagenet_dct", "train", num_ops=3, ops_magnitude=3, dtype=torch.float16, fused=False)
    rrc, flip, ra, tr = c.transforms
    assert ra.num_ops == 3 and tr.dtype == torch.float16
    for b in range(2):
        cy, cc = tr(ra(flip(rrc((dev(Yd[b]), dev(Cd[b])), box=boxes[b]), flip=flips[b]), ops=THREE[b]))
        assert cy.shape == (1, 28, 28, 8, 8) and same_bits(cy, fy[b]) and same_bits(cc, fc[b]), b
    torch.manual_seed(1)
    cy, cc = c((dev(Yd), dev(Cd)))
    assert cy.dtype == cc.dtype == torch.float16 and cy.shape == (2, 1, 28, 28, 8, 8) and cc.shape == (2, 2, 14, 14, 8, 8)
    assert float(cy.float().abs().max()) <= 1.0 and float(cc.float().abs().max()) <= 1.0


def test_randaugment_class_five_explicit_ops_in_one_pass():
    Y = detfill.integers((2, 1, 28, 28, 8, 8), 41, -1024, 1016)
    Cc = detfill.integers((2, 2, 14, 14, 8, 8), 42, -1024, 1016)
    ops = [("Cutout", 1.8, (6, 10)), ("Rotate90", 1.0, None), ("Equalize", 0.0, None), ("Solarize", 327.2, None),
           ("TranslateY", -3.75, None)]
    ra = CT.RandAugment_dct(num_ops=5, magnitude=3, ops_list=CT.DEFAULT_OPS)
    (oy, oc), names = KC.launched(lambda: ra((dev(Y), dev(Cc)), ops=ops))
    assert sum("dct_randaug" in n for n in names) == 1, names            # one pass, not three
    for b in range(2):
        ry, rc = np.clip(Y[b], -1024, 1016), np.clip(Cc[b], -1024, 1016)
        for name, mag, aux in ops:
            ry, rc = O.apply_op(ry, rc, name, mag, aux)
        assert np.array_equal(oy[b].cpu().numpy(), ry) and np.array_equal(oc[b].cpu().numpy(), rc)


# ================================================================================================== mixup
def fma32(c, l1, p):
    """fl32(c l1 + p) with ONE rounding, in numpy: the product of two fp32 values is exact in float64; the float64 sum is made
    with its exact error (TwoSum) and rounded to ODD where it is inexact, after which the rounding to fp32 is the correct one."""
    x, y = c.astype(np.float64) * np.float64(l1), p.astype(np.float64)
    s = x + y
    bb = s - x
    e = (x - (s - bb)) + (y - bb)                          # s + e == x + y exactly
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def mix_ref(x, lam, B):
    """The kernels' mix2 on the fp32 values of x [B, ...]: fp32 product a l0, then fma(c, l1, .) in fp32, c = the image before."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    p = a * np.float32(lam[0])
    assert p.dtype == np.float32
    return fma32(np.roll(a, 1, axis=0), np.float32(lam[1]), p)


@pytest.mark.parametrize("per", [4, 1028])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_mixup_any(B, per):
    lib = L.lib()
    lam_h = np.array([0.7315, 0.2685], np.float32)
    lam = dev(lam_h)
    x32 = torch.from_numpy(detfill.normalish((B, per), 90 + B)).to(DEV)
    st = L.stream()

    def call(entry, xin, odt, out=None):
        g = KC.guarded(B * per, None, odt) if out is None else out
        rc = entry(DT[xin.dtype], DT[odt], xin.data_ptr(), g.t.data_ptr(), lam.data_ptr(), B, per, st)
        torch.cuda.synchronize()
        return rc, g

    # the new pairs against fma in fp32 -> .half()
    for xin in (x32, x32.half()):
        rc, g = call(lib.rgbnm_mixup_any, xin, torch.float16)
        assert rc == 0
        g.check(f"mixup_any {xin.dtype} -> f16 B {B} per {per}")
        want = torch.from_numpy(mix_ref(xin.float().cpu().numpy(), lam_h, B)).half().reshape(-1)
        assert same_bits(g.t, want), (xin.dtype, B, per)
    # the old pairs: rgbnm_mixup's bits
    for xin, odt in ((x32, torch.float32), (x32, torch.bfloat16), (x32.bfloat16(), torch.bfloat16)):
        rc0, g0 = call(lib.rgbnm_mixup, xin, odt)
        rc1, g1 = call(lib.rgbnm_mixup_any, xin, odt)
        assert rc0 == rc1 == 0
        g1.check(f"mixup_any {xin.dtype} -> {odt}")
        assert torch.equal(g0.raw, g1.raw), (xin.dtype, odt)
    # refused pairs, and a row length that is no multiple of 4
    refused = [(x32.bfloat16(), torch.float32), (x32.half(), torch.float32), (x32.half(), torch.bfloat16),
               (x32.bfloat16(), torch.float16)]
    guards = [KC.guarded(B * per, None, odt) for _x, odt in refused] + [KC.guarded(B * per, None, torch.float16)]

    def fire():
        rcs = [lib.rgbnm_mixup_any(DT[x.dtype], DT[odt], x.data_ptr(), g.t.data_ptr(), lam.data_ptr(), B, per, st)
               for (x, odt), g in zip(refused, guards)]
        return rcs + [lib.rgbnm_mixup_any(0, 2, x32.data_ptr(), guards[-1].t.data_ptr(), lam.data_ptr(), B, per - 2, st)]
    rcs, names = KC.launched(fire)
    assert rcs == [EINVAL] * 5 and not names, (rcs, names)
    for g in guards:
        assert bool((g.raw == g.canary).all())


def test_random_mixup_on_fp16_items():
    B = 3
    y = torch.from_numpy(detfill.normalish((B, 1, 28, 28, 8, 8), 95)).to(DEV).half()
    c = torch.from_numpy(detfill.normalish((B, 2, 14, 14, 8, 8), 96)).to(DEV).half()
    lab = torch.tensor([3, 1, 7], device=DEV)
    mix = rg.cls_transforms.RandomMixup_DCT(10, alpha=0.2)
    lam = mix.sample_lambda(DEV)
    (my, mc), tgt = mix((y, c), lab, lam=lam)
    lam_h = lam.cpu().numpy()
    for got, x in ((my, y), (mc, c)):
        assert got.dtype == torch.float16
        assert same_bits(got, torch.from_numpy(mix_ref(x.float().cpu().numpy(), lam_h, B)).half())
    # fp32 items mixed to fp16, and the lazy item's materialize()
    mix.out_dtype = torch.float16
    (fy, _fc), _ = mix((y.float(), c.float()), lab, lam=lam)
    assert same_bits(fy, my)
    mix.out_dtype, mix.lazy = None, True
    (ly, _lc), _ = mix((y, c), lab, lam=lam)
    assert isinstance(ly, rg.cls_transforms.LazyMixed) and same_bits(ly.materialize(), my)


# ================================================================================================== model
def test_vit_step_fed_the_fp16_augment_output():
    """One ViT (E = 192, depth 1, B = 2) under autocast(float16) fed the fp16 augment output: forward and backward finite, logits
    against the fp32 mode fed the fp32 output of the same parameters.
    tests/test_fp16_model.py's bar for the E = 192 models is 1e-3 per logit, at depth 2 and 12 and B = 8; it has no number for this
    shape, so the bar is 1.5 x the deviation of the PARENT path -- the same fp16 model fed the fp32 output -- measured on an MI355X:
    PARENT_DEV = 3.853e-4 (max |logit| 0.794), bar 5.78e-4.  The margin is for the one extra rounding of 2^-11 per input
    coefficient.  The run under test measured 4.781e-4.  The parent path is measured again beside it and printed."""
    PARENT_DEV = 3.853e-4
    Y, Cc, quant = TA.synth(2, 40, 48, seed=33)
    params = [dict(box=(2, 4, 28, 28), flip=True, ops=THREE[0]), dict(box=(10, 16, 28, 28), flip=False, ops=THREE[1])]
    y16, c16 = CT.TrainTransform_DCT(out_dtype=torch.float16, num_ops=3)(dev(Y), dev(Cc), dev(quant), params=params)
    y32, c32 = CT.TrainTransform_DCT(out_dtype=torch.float32, num_ops=3)(dev(Y), dev(Cc), dev(quant), params=params)
    m = rg.ViT(3, 16, 192, depth=1, n_classes=1000, drop_p=0.0, device=DEV, num_heads=3, head_size=64, pixel_space="DCT", ver=1,
               use_subblock=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in detfill.fill_state_dict(shapes, base_seed=1).items()})
    t = detfill.uniform((2, 1000), 73, 0.0, 1.0)
    tgt = torch.from_numpy(t / t.sum(1, keepdims=True)).to(DEV)

    def step(y, c, dt):
        m.train()
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dt, enabled=dt != torch.float32):
            logits = m(y, c)
        loss = rg.cls_transforms.cross_entropy(logits, tgt, grad_dtype=dt)
        (loss * 2.0 ** 16).backward()
        torch.cuda.synchronize()
        return logits.detach().float().cpu().numpy(), loss.item(), [p.grad for p in m.parameters()]

    ref, _, _ = step(y32, c32, torch.float32)
    parent, _, _ = step(y32, c32, torch.float16)
    got, loss, grads = step(y16, c16, torch.float16)
    e_parent, e_got = float(np.abs(parent - ref).max()), float(np.abs(got - ref).max())
    print(f"max |dlogit| vs the fp32 mode: fp16 model fed fp32 {e_parent:.3e}, fed fp16 {e_got:.3e} (max |logit| {np.abs(ref).max():.3f})")
    assert np.isfinite(got).all() and np.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in grads)
    assert e_got <= 1e-3
    assert e_got <= 1.5 * PARENT_DEV
