#!/usr/bin/env python
"""Time the ViT training step (JPEG-Ti / JPEG-S, bf16) with dropout, in one process, alternating three configurations:

  drop      drop_p = P with train_dropout on: the per-block kernels with the dropout epilogues and apply launches
  drop_p0   drop_p = 2^-40 with train_dropout on: the same kernels and launches with threshold 0 and scale 1 (every element kept:
            the bits of p = 0), i.e. what the dropout path costs without dropping anything
  default   drop_p = 0: the default path (one-launch encoder), what bench.py times

A step is tools/fp16_step.py's: augment, lazy mixup, forward, soft-target loss, backward, fused clip + AdamW + weight decay.
WARMUP steps per configuration, then ROUNDS interleaved blocks timed with device events; every block starts from the initial
weights.  Prints one JSON line.  usage: python tools/dropout_step.py [--drop 0.1] [--steps 300] [--warmup 50] [--rounds 6]
[--arch vitti vits]
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
from rgb_no_more_amd import custom_transforms as CT  # noqa: E402
from bench import synth_coefficients  # noqa: E402

ARCH = {"vitti": (192, 3), "vits": (384, 6)}
CONFIGS = ("drop", "drop_p0", "default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--arch", nargs="+", default=["vitti", "vits"], choices=list(ARCH))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = a.batch
    res = {"batch": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "drop": a.drop}
    pdrop = {"drop": a.drop, "drop_p0": 2.0 ** -40, "default": 0.0}
    for arch in a.arch:
        emb, heads = ARCH[arch]
        torch.manual_seed(0)
        model = rg.ViT(3, 16, emb, depth=12, n_classes=1000, drop_p=0.0, device=dev, num_heads=heads, head_size=64,
                       pixel_space="DCT", ver=1, use_subblock=True)
        model.train_dropout = True
        model.train()
        opt = rg.custom_optims.FusedClipAdamWWD(model, lr=1e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)
        Yq, Cq, quant = synth_coefficients(B, dev, 1234)
        lab = torch.randint(0, 999, (B,), device=dev)
        aug = CT.TrainTransform_DCT(size=28, out_dtype=torch.bfloat16)
        sampler = CT.FastParamSampler(aug, seed=1234)
        mix = rg.cls_transforms.RandomMixup_DCT(1000, alpha=0.2)
        mix.out_dtype = torch.bfloat16
        mix.lazy, mix.lazy_target = True, True

        def step(cfg):
            model.drop_p = pdrop[cfg]
            packed, nops = sampler.sample(B, 64, 64)
            y, c = CT.apply_packed(aug, Yq, Cq, quant, packed, nops)
            lam = mix.sample_lambda(dev)
            (my, mc), mt = mix((y, c), lab, lam=lam)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = model(my, mc)
            loss = rg.cls_transforms.cross_entropy(logits, mt, grad_dtype=torch.bfloat16)
            loss.backward()
            opt.step()
            return loss

        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for cfg in CONFIGS:
            model.load_state_dict(state)
            for _ in range(a.warmup):
                step(cfg)
        torch.cuda.synchronize()
        ms = {cfg: [] for cfg in CONFIGS}
        per = max(1, a.steps // a.rounds)
        for r in range(a.rounds):
            for cfg in (CONFIGS if r % 2 == 0 else CONFIGS[::-1]):
                model.load_state_dict(state)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per):
                    step(cfg)
                e1.record()
                torch.cuda.synchronize()
                ms[cfg].append(e0.elapsed_time(e1) / per)
        out = {cfg: {"step_ms_median": float(np.median(v)), "step_ms_min": float(min(v)), "step_ms_max": float(max(v))}
               for cfg, v in ms.items()}
        out["drop_over_default"] = out["drop"]["step_ms_median"] / out["default"]["step_ms_median"]
        out["drop_over_drop_p0"] = out["drop"]["step_ms_median"] / out["drop_p0"]["step_ms_median"]
        res[arch] = out
        print(f"{arch}: " + ", ".join(f"{k} {v['step_ms_median']:.3f} ms" for k, v in out.items() if isinstance(v, dict)),
              file=sys.stderr)
        del model, opt
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
