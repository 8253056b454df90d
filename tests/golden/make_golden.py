"""Generate tests/golden/*.npz by IMPORTING THE REFERENCE (survey container only).

Run:  python tests/golden/make_golden.py
Needs /root/reference (read-only) and, for G1, oracle/_ref (python oracle/build_ref.py).
Nothing from the reference is copied: only input/output vectors are stored.  The reference's missing
third-party imports (torchvision, timm) are stubbed with empty modules; the stubbed symbols are only
dereferenced by functions that are out of scope.

Fixture index: G1 reader, G2 dequant, G3 conversion matrices, G4 geometric ops,
G5 resize, G6 photometric ops, G7 ToRange, G8 get_params, G9 sub-block embed, G10 sin-cos table,
G11 model fwd/bwd, G12 optimizer step, G13 mixup.
"""
import io
import os
import sys
import types
import math

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import rgb_no_more_amd as rg  # noqa: E402  (only detfill is used here)
from rgb_no_more_amd import detfill  # noqa: E402

REF = "/root/reference"


def _stub_modules():
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")

    class InterpolationMode:  # only referenced in signatures of out-of-scope RGB aug
        NEAREST = "nearest"
        BILINEAR = "bilinear"
        BICUBIC = "bicubic"

    tvt.InterpolationMode = InterpolationMode
    tvf.InterpolationMode = InterpolationMode
    tvt.functional = tvf
    tv.transforms = tvt
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt,
                        "torchvision.transforms.functional": tvf})
    # dct_manip python module name expected by custom_transforms
    from oracle import build_ref
    dm = build_ref.load_ref()
    if dm is not None:
        sys.modules["dct_manip"] = dm
    else:
        sys.modules["dct_manip"] = types.ModuleType("dct_manip")
    return dm


def main():
    torch.set_num_threads(4)
    dm = _stub_modules()
    sys.path.insert(0, REF)
    import utils.dct_ops as dops
    import utils.custom_transforms as ctrans
    import utils.cls_transforms as cls
    import utils.custom_optims as coptim
    import models.plainvit as pvit

    T = torch.from_numpy

    # ---------------- G1 reader -------------------------------------------------------------
    if dm is not None:
        from PIL import Image
        g1 = {}
        rng = np.random.default_rng(0)
        specs = [("c64x64", (64, 64), "RGB", 90, "4:2:0"), ("c48x80", (48, 80), "RGB", 90, "4:2:0"),
                 ("g40x56", (40, 56), "L", 75, None), ("c37x53", (37, 53), "RGB", 60, "4:2:0")]
        for name, (h, w), mode, q, ss in specs:
            small = rng.integers(0, 256, size=(max(h // 8, 2), max(w // 8, 2), 3), dtype=np.uint8)
            img = Image.fromarray(small, "RGB").resize((w, h), Image.BICUBIC)
            arr = np.asarray(img).astype(np.int16) + rng.normal(0, 6, size=(h, w, 3)).round().astype(np.int16)
            img = Image.fromarray(arr.clip(0, 255).astype(np.uint8), "RGB").convert(mode)
            buf = io.BytesIO()
            kw = dict(quality=q)
            if ss is not None:
                kw["subsampling"] = ss
            img.save(buf, format="JPEG", **kw)
            data = buf.getvalue()
            path = f"/tmp/_g1_{name}.jpg"
            with open(path, "wb") as f:
                f.write(data)
            dim, quant, Y, cbcr = dm.read_coefficients(path)
            g1[name + "_jpeg"] = np.frombuffer(data, dtype=np.uint8)
            g1[name + "_dim"] = dim.numpy()
            g1[name + "_quant"] = quant.numpy()
            g1[name + "_Y"] = Y.numpy()
            if cbcr is not None:
                g1[name + "_CbCr"] = cbcr.numpy()
        np.savez_compressed(os.path.join(HERE, "g1_reader.npz"), **g1)
        print("G1 ok", {k: v.shape for k, v in g1.items() if k.endswith("_Y")})
    else:
        print("G1 skipped (oracle/_ref not built)")

    # ---------------- G2 dequant (datasets.py:288-293 expression, torch int16 semantics) -----
    Y = detfill.integers((1, 3, 3, 8, 8), 11, -1200, 1200)
    C = detfill.integers((2, 2, 2, 8, 8), 12, -600, 600)
    quant = detfill.integers((3, 8, 8), 13, 1, 99)
    quant[0, 0, 0] = 255
    Y[0, 0, 0, 0, 0] = 1000  # 1000*255 wraps in int16
    Y[0, 0, 1, 0, 0] = -300
    tY, tC, tq = T(Y), T(C), T(quant)
    oY = torch.clamp(tY * tq[0], min=-2**10, max=2**10 - 8)
    oC = torch.clamp(tC * tq[1:3].unsqueeze(1).unsqueeze(1), min=-2**10, max=2**10 - 8)
    np.savez_compressed(os.path.join(HERE, "g2_dequant.npz"), Y=Y, C=C, quant=quant,
                        oY=oY.numpy(), oC=oC.numpy())

    # ---------------- G3 conversion matrices -----------------------------------------------
    g3 = {}
    for ls, m in [(8, 2), (4, 2), (2, 4), (8, 1)]:
        g3[f"A_{ls}_{m}"] = dops.generate_conversion_matrix(ls, m).numpy()
        g3[f"A64_{ls}_{m}"] = dops.generate_conversion_matrix(ls, m, dtype=torch.float64).numpy()
    g3["basis8"] = dops.generate_basis_matrix(8).numpy()
    np.savez_compressed(os.path.join(HERE, "g3_convmat.npz"), **g3)

    # ---------------- G4 geometric / masking ops (bit-exact) -------------------------------
    g4 = {}
    Y = detfill.integers((1, 6, 8, 8, 8), 21, -1024, 1016)
    C = detfill.integers((2, 3, 4, 8, 8), 22, -1024, 1016)
    g4["Y"], g4["C"] = Y, C
    tY, tC = T(Y), T(C)
    g4["crop_Y_2_2_4_4"] = dops.crop_dct(tY, 2, 2, 4, 4).contiguous().numpy()
    g4["crop_C_1_1_2_2"] = dops.crop_dct(tC, 1, 1, 2, 2).contiguous().numpy()
    g4["flipH_Y"] = dops.flip_dct(tY, "horizontal").numpy()
    g4["flipH_C"] = dops.flip_dct(tC, "horizontal").numpy()
    g4["flipV_Y"] = dops.flip_dct(tY, "vertical").numpy()
    for r in (-1, 1, 2, 3, -3, 4):
        g4[f"rot{r}_Y"] = dops.rotate_dct_90deg(tY, rotate=r).contiguous().numpy()
        g4[f"rot{r}_C"] = dops.rotate_dct_90deg(tC, rotate=r).contiguous().numpy()
    for mag in (2, -4):
        for d in ("H", "W"):
            g4[f"trans{d}{mag}_Y"] = dops.translate_dct(tY, mag, d).numpy()
            g4[f"trans{d}{mag}_C"] = dops.translate_dct(tC, mag // 2, d).numpy()
    for (ch, cw) in [(0, 0), (2, 4), (4, 6)]:
        oy, _, _ = dops.cutout_dct(tY, 2, 0, ch, cw)
        oc, _, _ = dops.cutout_dct(tC, 1, 0, ch // 2, cw // 2)
        g4[f"cutout_{ch}_{cw}_Y"] = oy.numpy()
        g4[f"cutout_{ch}_{cw}_C"] = oc.numpy()
    np.savez_compressed(os.path.join(HERE, "g4_geom.npz"), **g4)

    # ---------------- G5 resize (fp32 and fp64 reference runs) ------------------------------
    g5 = {}
    Y = detfill.integers((1, 4, 4, 8, 8), 31, -1024, 1016)
    Y[..., 4:, :] //= 8
    Y[..., :, 4:] //= 8   # JPEG-like energy decay
    C = detfill.integers((2, 2, 2, 8, 8), 32, -1024, 1016)
    g5["Y"], g5["C"] = Y, C
    for nm, arr in (("Y", Y), ("C", C)):
        t = T(arr)
        hb = arr.shape[1]
        for size in (hb * 2, hb, hb // 2):
            g5[f"{nm}_to{size}_f32"] = dops.resize_dct(t, size, dtype=torch.float32, conv_mxs={}).numpy()
            # fp64 pre-round values to mark ties
            up, _, _ = dops.upsample_dct(t, L=size // math.gcd(hb, size), M=size // math.gcd(hb, size), dtype=torch.float64)
            dn, _, _ = dops.downsample_dct(up, L=hb // math.gcd(hb, size), M=hb // math.gcd(hb, size), dtype=torch.float64)
            g5[f"{nm}_to{size}_f64raw"] = dn.numpy()
    np.savez_compressed(os.path.join(HERE, "g5_resize.npz"), **g5)

    # ---------------- G6 photometric ops + RandAugment dispatcher at vitti magnitudes --------
    g6 = {}
    Y = detfill.integers((1, 6, 6, 8, 8), 41, -1024, 1016)
    Y[..., 0, 0] = detfill.integers((1, 6, 6), 43, -900, 900)
    C = detfill.integers((2, 3, 3, 8, 8), 42, -1024, 1016)
    g6["Y"], g6["C"] = Y, C
    ra = ctrans.RandAugment_dct(num_ops=2, magnitude=3, num_magnitude_bins=11, ops_list=["Identity"])
    meta = ra._augmentation_space(11, (6, 6))
    mags = {}
    for k, (m, signed) in meta.items():
        mags[k] = float(m[3].item()) if m.ndim > 0 else float(m.item())
    g6["mag_names"] = np.array(list(mags.keys()))
    g6["mag_vals"] = np.array(list(mags.values()), dtype=np.float64)
    meta28 = ra._augmentation_space(11, (28, 28))
    g6["mag_translate_28"] = np.float64(meta28["TranslateX"][0][3].item())
    ops = ["AutoContrast", "Posterize", "SolarizeAdd", "Color", "Contrast", "Brightness", "MidfreqAug",
           "TranslateX", "TranslateY", "Rotate90", "AutoSaturation", "Grayscale", "Sharpness", "Identity"]
    for op in ops:
        m, signed = meta[op]
        mag = float(m[3].item()) if m.ndim > 0 else m.item()
        for sgn in ((1.0, -1.0) if signed else (1.0,)):
            coeff = [T(Y).clone(), T(C).clone()]
            out = ctrans._apply_op_dct(coeff, op, mag * sgn, pad=2**0.5, conv_Ls=[None, None], conv_Ms=[None, None])
            tag = f"{op}_{'p' if sgn > 0 else 'n'}"
            g6[tag + "_Y"] = out[0].numpy()
            g6[tag + "_C"] = out[1].numpy()
            g6[tag + "_mag"] = np.float64(mag * sgn)
    # Cutout / ChromaDrop draw from torch RNG inside: pin with seeds and record the draws
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        coeff = [T(Y).clone(), T(C).clone()]
        out = ctrans._apply_op_dct(coeff, "Cutout", mags["Cutout"], pad=2**0.5, conv_Ls=[None, None], conv_Ms=[None, None])
        torch.manual_seed(seed)
        ch = (torch.randint(low=0, high=6, size=(1,)).item()) // 2 * 2
        cw = (torch.randint(low=0, high=6, size=(1,)).item()) // 2 * 2
        g6[f"Cutout_s{seed}_Y"], g6[f"Cutout_s{seed}_C"] = out[0].numpy(), out[1].numpy()
        g6[f"Cutout_s{seed}_center"] = np.array([ch, cw])
        torch.manual_seed(seed)
        coeff = [T(Y).clone(), T(C).clone()]
        out = ctrans._apply_op_dct(coeff, "ChromaDrop", 0.0, pad=2**0.5, conv_Ls=[None, None], conv_Ms=[None, None])
        torch.manual_seed(seed)
        drop_cb = torch.rand(1).item() > 0.5
        g6[f"ChromaDrop_s{seed}_C"] = out[1].numpy()
        g6[f"ChromaDrop_s{seed}_dropcb"] = np.array(int(drop_cb))
    # flat-DC edge cases for autocontrast
    Yz = Y.copy()
    Yz[..., 0, 0] = 0
    g6["AutoContrast_zero_in"] = Yz
    g6["AutoContrast_zero_out"] = dops.autocontrast_dct(T(Yz)).numpy()
    np.savez_compressed(os.path.join(HERE, "g6_photo.npz"), **g6)

    # ---------------- G7 ToRange --------------------------------------------------------------
    x = detfill.integers((1, 2, 2, 8, 8), 51, -1024, 1016)
    x.reshape(-1)[:4] = [-1024, 1016, 0, -4]
    tr = ctrans.ToRange(val_min=-1, val_max=1, orig_min=-1024, orig_max=1016, dtype=torch.float32)
    np.savez_compressed(os.path.join(HERE, "g7_torange.npz"), x=x, out=tr(T(x)).numpy())

    # ---------------- G8 RandomResizedCrop_DCT.get_params ------------------------------------
    rows = []
    for size, grid in ((28, (64, 64)), (28, (47, 63)), (32, (64, 64)), (28, (28, 28)), (28, (100, 80))):
        rrc = ctrans.RandomResizedCrop_DCT(size, scale=(0.05, 1.0), ratio=(1, 1))
        dummy = torch.zeros((1, grid[0], grid[1], 1, 1), dtype=torch.int16)
        for seed in range(40):
            torch.manual_seed(seed)
            i, j, h, w = rrc.get_params(dummy, rrc.scale, rrc.ratio, rrc.even_size_choices, 2)
            # replay raw draws (valid when the first of the 10 attempts succeeds, which we check)
            torch.manual_seed(seed)
            u = torch.empty(1).uniform_(0.05, 1.0).item()
            ri = int(torch.randint(0, grid[0] - h + 1, size=(1,)).item()) if h <= grid[0] else -1
            rj = int(torch.randint(0, grid[1] - w + 1, size=(1,)).item()) if w <= grid[1] else -1
            first_ok = (ri // 2 * 2 == i) and (rj // 2 * 2 == j)
            rows.append([size, grid[0], grid[1], seed, u, ri, rj, i, j, h, w, int(first_ok)])
    g8 = np.array(rows, dtype=np.float64)
    # eval transform ResizedCenterCrop_DCT(32, 28).get_params
    rcc = ctrans.ResizedCenterCrop_DCT(32, 28)
    ev = []
    for grid in ((64, 64), (47, 63), (100, 80), (32, 32)):
        d1 = torch.zeros((1, grid[0], grid[1], 1, 1), dtype=torch.int16)
        ev.append([grid[0], grid[1], *rcc.get_params(d1, 2)])
    np.savez_compressed(os.path.join(HERE, "g8_params.npz"), rrc=g8, rcc=np.array(ev, dtype=np.int64))

    # ---------------- G9 sub-block embed (pre-projection features) ----------------------------
    pe = pvit.PatchEmbedding_DCT_Group(16, 192, True)
    y = detfill.normalish((2, 1, 4, 6, 8, 8), 61)
    c = detfill.normalish((2, 2, 2, 3, 8, 8), 62)
    ty, tc = T(y), T(c)
    yy = pvit.apply_subblock(pe.rearrange_Y(ty), pe.conv_Y, combine=True)
    feat = torch.cat([pe.collapser(yy), pe.collapser(pe.rearrange_C(tc))], dim=3)
    np.savez_compressed(os.path.join(HERE, "g9_subblock.npz"), feat=feat.numpy(), convY=pe.conv_Y.numpy())

    # ---------------- G10 sin-cos table: make_golden_sincos.py (MKL's reproducible mode, set before torch starts) -------------

    # ---------------- G11 model forward/backward ----------------------------------------------
    g11 = {}
    for tag, emb, heads, depth, B in (("ti_d2", 192, 3, 2, 2), ("ti_d12", 192, 3, 12, 4), ("s_d2", 384, 6, 2, 2)):
        model = pvit.ViT(3, 16, emb, depth=depth, n_classes=1000, drop_p=0.0, device="cpu",
                         num_heads=heads, head_size=64, pixel_space="DCT", ver=1, use_subblock=True)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = detfill.fill_state_dict(shapes, base_seed=1)
        model.load_state_dict({k: T(v) for k, v in sd.items()})
        model.train()
        y = detfill.normalish((B, 1, 28, 28, 8, 8), 71)
        c = detfill.normalish((B, 2, 14, 14, 8, 8), 72)
        tgt = detfill.uniform((B, 1000), 73, 0.0, 1.0)
        tgt = tgt / tgt.sum(1, keepdims=True)
        ty, tc, tt = T(y), T(c), T(tgt)
        # intermediate activations
        x0 = model.patchembed(ty, tc)
        x1 = model.encoder[0](x0.clone())
        logits = model(ty, tc)
        loss = torch.nn.CrossEntropyLoss()(logits, tt)
        loss.backward()
        g11[tag + "_names"] = np.array(list(shapes.keys()))
        g11[tag + "_x0_slice"] = x0.detach()[:, ::49, ::16].numpy()
        g11[tag + "_x1_slice"] = x1.detach()[:, ::49, ::16].numpy()
        g11[tag + "_logits"] = logits.detach().numpy()
        g11[tag + "_loss"] = np.float64(loss.item())
        gn = np.array([p.grad.double().norm().item() for _, p in model.named_parameters()])
        g11[tag + "_gradnorms"] = gn
        named = dict(model.named_parameters())
        for nm in ("patchembed.projection.0.weight", "encoder.0.0.fn.eb_mha.qkv.weight", "encoder.0.0.fn.eb_mha.qkv.bias",
                   "encoder.1.1.fn.eb_ffb.3.weight", "encoder.0.0.fn.eb_lrnorm1.weight", "classhead.ch_linear2.bias"):
            g11[tag + "_grad_" + nm] = named[nm].grad.reshape(-1)[::37].numpy().copy()
        # int labels variant (benchmark.py semantics)
        model.zero_grad()
        lab = torch.from_numpy(detfill.integers((B,), 74, 0, 998, np.int64))
        l2 = torch.nn.CrossEntropyLoss()(model(ty, tc), lab)
        g11[tag + "_loss_int"] = np.float64(l2.item())
        print("G11", tag, "loss", loss.item(), "logit absmax", logits.abs().max().item())
    np.savez_compressed(os.path.join(HERE, "g11_model.npz"), **g11)

    # ---------------- G12 optimizer step (clip + AdamW(wd=0) + WeightDecay) --------------------
    g12 = {}
    names = ["a.weight", "a.bias", "x_lrnorm.weight", "b.weight"]
    shapes = [(5, 7), (5,), (7,), (3, 5)]
    params = [torch.nn.Parameter(T(detfill.uniform(s, 81 + i))) for i, s in enumerate(shapes)]
    for it in range(3):
        for i, p in enumerate(params):
            p.grad = T(detfill.uniform(shapes[i], 91 + 10 * it + i, -2.0, 2.0))
    opt = torch.optim.AdamW(params, lr=3e-3, weight_decay=0, eps=1e-8)
    wdp = [p for n, p in zip(names, params) if (".weight" in n) and ("lrnorm" not in n)]
    wd = coptim.WeightDecay(wdp, lr=3e-3, weight_decay=1e-4)
    g12["p0"] = np.concatenate([p.detach().numpy().reshape(-1) for p in params])
    lrs = [3e-3, 1.5e-3, 2.5e-3]
    for it in range(3):
        for i, p in enumerate(params):
            p.grad = T(detfill.uniform(shapes[i], 91 + 10 * it + i, -2.0, 2.0))
        for g in opt.param_groups:
            g["lr"] = lrs[it]
        for g in wd.param_groups:
            g["lr"] = lrs[it]
        tn = torch.nn.utils.clip_grad_norm_(params, max_norm=1)
        opt.step()
        wd.step()
        g12[f"p{it + 1}"] = np.concatenate([p.detach().numpy().reshape(-1) for p in params])
        g12[f"norm{it + 1}"] = np.float64(tn.item())
    np.savez_compressed(os.path.join(HERE, "g12_optim.npz"), **g12)

    # ---------------- G13 mixup ----------------------------------------------------------------
    mix = cls.RandomMixup_DCT(10, alpha=0.2)
    y = detfill.normalish((4, 1, 2, 2, 8, 8), 101)
    c = detfill.normalish((4, 2, 1, 1, 8, 8), 102)
    lab = torch.tensor([1, 3, 3, 7])
    torch.manual_seed(5)
    (my, mc), mt = mix((T(y), T(c)), lab)
    torch.manual_seed(5)
    lam, _ = torch._sample_dirichlet(torch.tensor([0.2, 0.2])).sort(descending=True)
    np.savez_compressed(os.path.join(HERE, "g13_mixup.npz"), y=y, c=c, lab=lab.numpy(), lam=lam.numpy(),
                        my=my.numpy(), mc=mc.numpy(), mt=mt.numpy())
    print("done")


if __name__ == "__main__":
    main()
