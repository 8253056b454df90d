#!/usr/bin/env python
"""Time the training step of the ViT (JPEG-Ti / JPEG-S) or of SwinV2-T in its compute configurations, in one process,
alternating (--configs picks them; default: the first four, what profiles/fp16_tuned_step.json holds):

  fp16          autocast(float16) with the library's defaults: fp16 activations on the generic kernels
  fp16_tuned    autocast(float16) with the option f16_tuned = 1: the plain GEMMs (small-M, weight-resident, row-panel, pipelined and
                grouped weight gradients) on the kernels tuned for 16-bit operands; SwinV2-T: also group_dw_backward + hold_reductions
  bf16_generic  bf16 with exactly the bf16-only kernels switched off (BF16_ONLY_OPTS; SwinV2-T: also the backward-wide weight-
                gradient bracket and the held reductions, group_dw_backward): the kernel set fp16 runs
  bf16          bf16 with every option at its default (what bench.py times; SwinV2-T: group_dw_backward + hold_reductions on,
                drop_path_rate 0.2, as bench.py --arch swinv2t)
  fp16_fused    autocast(float16) with f16_tuned = 2: fp16_tuned plus attention v2, the fused MLP and the LayerNorm-chained epilogues
                in fp16 -- the whole per-block tuned path
  bf16_nochain  bf16 with fwd_chain = bwd_chain = 0: the kernel set of fp16_fused, in bf16
  fp16_fused_noattn / _nomlp / _noln   fp16_fused with one family switched off (attn_v2 | mlp_fuse + mlp_bwd | ln_fuse; the fused
                MLP backward needs ln_fuse and goes with it): the per-family A/B

A step is what bench.py times, launched eagerly: augment (DCT-domain, fp32 output for fp16 and bf16_generic, bf16 for bf16),
lazy mixup, forward, soft-target loss, backward, fused clip + AdamW + weight decay.  Per arch, every configuration runs WARMUP
steps, then the timed steps in ROUNDS interleaved blocks (device events around each block, after a synchronise); every block
starts from the initial weights (the step has no loss scaler, and the weights must stay where fp16 activations fit).  Also reports
the max |logit - reference| at B = 256 per configuration: JPEG-Ti depth 12 (golden g20) for the ViT archs, SwinV2-T (golden g21)
for swinv2t -- the reference models on detfill weights.
Prints one JSON line.  usage: python tools/fp16_step.py [--steps 300] [--warmup 50] [--rounds 6] [--arch vitti vits swinv2t]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rgb_no_more_amd as rg  # noqa: E402
from rgb_no_more_amd import custom_transforms as CT, detfill, lib as L  # noqa: E402
from bench import synth_coefficients  # noqa: E402

ARCH = {"vitti": (192, 3), "vits": (384, 6), "swinv2t": (96, 3)}
# every library option that selects a kernel fp16 does not reach under default options: bf16-only kernels, and the tuned plain GEMMs
# (nt_kpipe, nt_wres, nt_small, tn_pipe, tn_wide) that fp16 takes only with f16_tuned = 1
BF16_ONLY_OPTS = ("fwd_chain", "bwd_chain", "nt_kpipe", "nt_wres", "nt_small", "tn_pipe", "tn_wide", "mlp_fuse", "mlp_bwd",
                  "attn_v2", "ln_fuse")
CONFIGS = ("fp16", "fp16_tuned", "bf16_generic", "bf16")
# name -> (f16_tuned level, options switched off on top of the defaults)
EXTRA = {"fp16_fused": (2, ()), "bf16_nochain": (0, ("fwd_chain", "bwd_chain")), "fp16_fused_noattn": (2, ("attn_v2",)),
         "fp16_fused_nomlp": (2, ("mlp_fuse", "mlp_bwd")), "fp16_fused_noln": (2, ("ln_fuse",))}
F16_CONFIGS = ("fp16", "fp16_tuned") + tuple(k for k in EXTRA if k.startswith("fp16"))
TUNED_SETS = ("bf16", "bf16_nochain", "fp16_tuned") + tuple(k for k in EXTRA if k.startswith("fp16"))


def set_opts(defaults, off, f16_tuned=0, also_off=()):
    lib = L.lib()
    lib.rgbnm_set_option(b"f16_tuned", f16_tuned)
    for k, v in defaults.items():
        lib.rgbnm_set_option(k.encode(), 0 if ((off and k in BF16_ONLY_OPTS) or k in also_off) else v)


def set_cfg(defaults, cfg):
    level, also_off = EXTRA.get(cfg, (int(cfg == "fp16_tuned"), ()))
    set_opts(defaults, cfg == "bf16_generic", level, also_off)


def swin_model(dev, drop_path_rate):
    return rg.SwinTransformerV2(img_size=256, patch_size=4, embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                                window_size=8, drop_path_rate=drop_path_rate, device=dev, pixel_space="dct")


def swin_logit_error(cfg, defaults):
    """max |logit - reference| of SwinV2-T, B = 256 (tests/golden/g21_b256.npz; the fill of bench.py's parity check)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g21_b256.npz"))
    m = swin_model("cuda", 0.0)
    names = [str(n) for n in g["swt_b256_names"]]
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in detfill.fill_swin_params({n: shapes[n] for n in names}).items()},
                      strict=False)
    y = torch.from_numpy(detfill.normalish((256, 1, 32, 32, 8, 8), 171)).cuda()
    c = torch.from_numpy(detfill.normalish((256, 2, 16, 16, 8, 8), 172)).cuda()
    set_cfg(defaults, cfg)
    m.train()
    with torch.autocast("cuda", dtype=torch.float16 if cfg in F16_CONFIGS else torch.bfloat16):
        out = m(y, c)
    torch.cuda.synchronize()
    set_opts(defaults, False)
    return float(np.abs(out.detach().float().cpu().numpy() - g["swt_b256_logits"]).max())


def logit_error(cfg, defaults):
    """max |logit - reference| of JPEG-Ti, depth 12, B = 256 (tests/golden/g20_fullsize.npz)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g20_fullsize.npz"))
    m = rg.ViT(3, 16, 192, depth=12, n_classes=1000, drop_p=0.0, device="cuda", num_heads=3, head_size=64, pixel_space="DCT", ver=1)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in detfill.fill_state_dict(shapes, base_seed=1).items()})
    y = torch.from_numpy(detfill.normalish((256, 1, 28, 28, 8, 8), 71)).cuda()
    c = torch.from_numpy(detfill.normalish((256, 2, 14, 14, 8, 8), 72)).cuda()
    set_cfg(defaults, cfg)
    m.train()
    with torch.autocast("cuda", dtype=torch.float16 if cfg in F16_CONFIGS else torch.bfloat16):
        out = m(y, c)
    torch.cuda.synchronize()
    set_opts(defaults, False)
    return float(np.abs(out.detach().float().cpu().numpy() - g["ti_d12_b256_logits"]).max())


def main():
    global CONFIGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--arch", nargs="+", default=["vitti", "vits"], choices=list(ARCH))
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS) + list(EXTRA))
    a = ap.parse_args()
    CONFIGS = tuple(a.configs)
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    defaults = {k: lib.rgbnm_get_option(k.encode()) for k in BF16_ONLY_OPTS}
    res_configs = list(CONFIGS)
    print(f"bf16_generic: options switched off: {', '.join(BF16_ONLY_OPTS)}", file=sys.stderr)
    B = a.batch
    res = {"batch": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "bf16_only_options_off": list(BF16_ONLY_OPTS),
           "configs": res_configs}
    for arch in a.arch:
        emb, heads = ARCH[arch]
        torch.manual_seed(0)
        swin = arch == "swinv2t"
        if swin:
            model = swin_model(dev, 0.2)
        else:
            model = rg.ViT(3, 16, emb, depth=12, n_classes=1000, drop_p=0.0, device=dev, num_heads=heads, head_size=64,
                           pixel_space="DCT", ver=1, use_subblock=True)
        model.train()
        opt = rg.custom_optims.FusedClipAdamWWD(model, lr=1e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)
        Yq, Cq, quant = synth_coefficients(B, dev, 1234)
        lab = torch.randint(0, 999, (B,), device=dev)
        legs = {}
        for cfg in CONFIGS:
            adt = torch.bfloat16 if cfg == "bf16" else torch.float32          # augment output (fed float16 instead: tools/aug_chain_step.py)
            cdt = torch.float16 if cfg in F16_CONFIGS else torch.bfloat16
            aug = CT.TrainTransform_DCT(size=32 if swin else 28, out_dtype=adt)
            mix = rg.cls_transforms.RandomMixup_DCT(1000, alpha=0.2)
            mix.out_dtype = adt
            mix.lazy, mix.lazy_target = True, True
            legs[cfg] = (aug, CT.FastParamSampler(aug, seed=1234), mix, cdt)

        def configure(cfg):
            set_cfg(defaults, cfg)
            if swin:                            # the backward-wide bracket and the held reductions: on the tuned kernel sets only
                model.group_dw_backward = model.hold_reductions = cfg in TUNED_SETS

        def step(cfg):
            aug, sampler, mix, cdt = legs[cfg]
            packed, nops = sampler.sample(B, 64, 64)
            y, c = CT.apply_packed(aug, Yq, Cq, quant, packed, nops)
            lam = mix.sample_lambda(dev)
            (my, mc), mt = mix((y, c), lab, lam=lam)
            with torch.autocast("cuda", dtype=cdt):
                logits = model(my, mc)
            loss = rg.cls_transforms.cross_entropy(logits, mt, grad_dtype=cdt)
            loss.backward()
            opt.step()
            return loss

        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for cfg in CONFIGS:
            configure(cfg)
            model.load_state_dict(state)
            for _ in range(a.warmup):
                step(cfg)
        torch.cuda.synchronize()
        ms = {cfg: [] for cfg in CONFIGS}
        nonfinite = {cfg: 0 for cfg in CONFIGS}      # timed blocks whose last loss was not finite
        per = max(1, a.steps // a.rounds)
        for r in range(a.rounds):
            for cfg in (CONFIGS if r % 2 == 0 else CONFIGS[::-1]):
                configure(cfg)
                model.load_state_dict(state)    # every block from the same weights (no loss scaler here: keep fp16 in range)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per):
                    loss = step(cfg)
                e1.record()
                torch.cuda.synchronize()
                if not torch.isfinite(loss).item():
                    nonfinite[cfg] += 1
                ms[cfg].append(e0.elapsed_time(e1) / per)
        set_opts(defaults, False)
        model.load_state_dict(state)
        out = {cfg: {"step_ms_median": float(np.median(v)), "step_ms_min": float(min(v)), "step_ms_max": float(max(v)),
                     "nonfinite_blocks": nonfinite[cfg]} for cfg, v in ms.items()}
        for num, den in (("fp16", "bf16_generic"), ("fp16", "bf16"), ("fp16_tuned", "fp16"), ("fp16_tuned", "bf16"),
                         ("fp16_fused", "fp16_tuned"), ("fp16_fused", "bf16_nochain"), ("fp16_fused", "bf16")):
            if num in ms and den in ms:
                out[f"{num}_over_{den}"] = out[num]["step_ms_median"] / out[den]["step_ms_median"]
        res[arch] = out
        print(f"{arch}: " + ", ".join(f"{k} {v['step_ms_median']:.3f} ms" for k, v in out.items() if isinstance(v, dict)), file=sys.stderr)
        del model, opt
        torch.cuda.empty_cache()
    if any(x != "swinv2t" for x in a.arch):
        res["max_abs_dlogit_ti_b256"] = {cfg: logit_error(cfg, defaults) for cfg in CONFIGS}
    if "swinv2t" in a.arch:
        res["max_abs_dlogit_swinv2t_b256"] = {cfg: swin_logit_error(cfg, defaults) for cfg in CONFIGS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
