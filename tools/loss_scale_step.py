#!/usr/bin/env python
"""Time the fp16 training step (JPEG-Ti, SwinV2-T; B = 256; option f16_tuned = 1) under a loss scaler, two ways, in one
process, alternating:

  A  stock torch around the fused tail: torch.amp.GradScaler(1.6, 0.625, 600).scale(loss).backward(), unscale_(optimizer),
     scaler.step(FusedClipAdamWWD), update(), the reference's clip_gradscaler (pipeline_utils.py:399-409) -- what fp16 training
     on the fused tail costs without DeviceLossScaler: extra passes over the gradients and two host syncs per step
  B  custom_optims.DeviceLossScaler: scale(loss).backward(), step(optimizer), update() -- the scaler inside the tail's two launches

A step is what tools/fp16_step.py times: augment, lazy mixup, forward under autocast(float16), soft-target loss, backward, tail.
Both paths warm up, then run the timed steps in ROUNDS interleaved blocks (device events around each block, which ends in a
synchronise); every block starts from the same weights, moments and scaler state.  Launches per step are counted with
torch.profiler over a few extra steps after the timing.
Writes profiles/loss_scale_step.json and prints it.
usage: python tools/loss_scale_step.py [--steps 300] [--warmup 50] [--rounds 6] [--arch vitti swinv2t]
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rgb_no_more_amd as rg  # noqa: E402
from rgb_no_more_amd import custom_transforms as CT, lib as L  # noqa: E402
from rgb_no_more_amd.custom_optims import DeviceLossScaler, FusedClipAdamWWD  # noqa: E402
from bench import synth_coefficients  # noqa: E402

ARCH = {"vitti": (192, 3), "swinv2t": (96, 3)}
PATHS = ("A", "B")


def clip_gradscaler(gradscaler, scale_max=2 ** 18, scale_min=2 ** (-4)):
    """pipeline_utils.py:399-409 semantics (each comparison syncs the host)."""
    if gradscaler._scale > scale_max:
        gradscaler._scale = torch.tensor(scale_max).to(gradscaler._scale)
    if gradscaler._scale < scale_min:
        gradscaler._scale = torch.tensor(scale_min).to(gradscaler._scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--arch", nargs="+", default=["vitti", "swinv2t"], choices=list(ARCH))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_scale_step.json"))
    ap.add_argument("--f16-tuned", type=int, default=1, choices=(1, 2), help="level of the option f16_tuned")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = L.lib()
    tuned0 = lib.rgbnm_get_option(b"f16_tuned")
    lib.rgbnm_set_option(b"f16_tuned", a.f16_tuned)
    B = a.batch
    res = {"batch": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "dtype": "float16", "f16_tuned": a.f16_tuned,
           "source_hash": L.source_hash()}
    for arch in a.arch:
        emb, heads = ARCH[arch]
        torch.manual_seed(0)
        swin = arch == "swinv2t"
        if swin:
            model = rg.SwinTransformerV2(img_size=256, patch_size=4, embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                                         window_size=8, drop_path_rate=0.2, device=dev, pixel_space="dct")
            model.group_dw_backward = model.hold_reductions = True      # as tools/fp16_step.py's fp16_tuned leg
        else:
            model = rg.ViT(3, 16, emb, depth=12, n_classes=1000, drop_p=0.0, device=dev, num_heads=heads, head_size=64,
                           pixel_space="DCT", ver=1, use_subblock=True)
        model.train()
        opt = FusedClipAdamWWD(model, lr=1e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)
        Yq, Cq, quant = synth_coefficients(B, dev, 1234)
        lab = torch.randint(0, 999, (B,), device=dev)
        aug = CT.TrainTransform_DCT(size=32 if swin else 28, out_dtype=torch.float32)
        mix = rg.cls_transforms.RandomMixup_DCT(1000, alpha=0.2)
        mix.out_dtype = torch.float32
        mix.lazy, mix.lazy_target = True, True
        samplers = {p: CT.FastParamSampler(aug, seed=1234) for p in PATHS}
        scalers = {"A": torch.amp.GradScaler("cuda", growth_factor=1.6, backoff_factor=0.625, growth_interval=600),
                   "B": DeviceLossScaler()}

        def step(path):
            packed, nops = samplers[path].sample(B, 64, 64)
            y, c = CT.apply_packed(aug, Yq, Cq, quant, packed, nops)
            lam = mix.sample_lambda(dev)
            (my, mc), mt = mix((y, c), lab, lam=lam)
            with torch.autocast("cuda", dtype=torch.float16):
                logits = model(my, mc)
            loss = rg.cls_transforms.cross_entropy(logits, mt, grad_dtype=torch.float16)
            s = scalers[path]
            s.scale(loss).backward()
            if path == "A":
                s.unscale_(opt)
                s.step(opt)
                s.update()
                clip_gradscaler(s)
            else:
                s.step(opt)
                s.update()
            return loss

        weights = {k: v.detach().clone() for k, v in model.state_dict().items()}
        opt_state = copy.deepcopy(opt.state_dict())
        scaler_state = {"scale": 65536.0, "growth_factor": 1.6, "backoff_factor": 0.625, "growth_interval": 600,
                        "_growth_tracker": 0}

        def restart(path):                       # the same weights, moments, step count and scale for every block
            model.load_state_dict(weights)
            opt.load_state_dict(copy.deepcopy(opt_state))
            scalers[path].load_state_dict(dict(scaler_state))

        for path in PATHS:
            restart(path)
            for _ in range(a.warmup):
                step(path)
        torch.cuda.synchronize()
        ms = {p: [] for p in PATHS}
        nonfinite = {p: 0 for p in PATHS}
        end = {}
        per = max(1, a.steps // a.rounds)
        for r in range(a.rounds):
            for path in (PATHS if r % 2 == 0 else PATHS[::-1]):
                restart(path)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per):
                    loss = step(path)
                e1.record()
                torch.cuda.synchronize()
                if not torch.isfinite(loss).item():
                    nonfinite[path] += 1
                ms[path].append(e0.elapsed_time(e1) / per)
                taken = int(float(opt.state_dict()["state"][0]["step"]))
                end[path] = {"scale": scalers[path].get_scale(), "steps_taken": taken, "steps_skipped": per - taken}
        launches = {}
        from torch.profiler import profile, ProfilerActivity
        for path in PATHS:
            restart(path)
            step(path)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(4):
                    step(path)
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
            launches[path] = n / 4
        out = {p: {"step_ms_median": float(np.median(ms[p])), "step_ms_min": float(min(ms[p])), "step_ms_max": float(max(ms[p])),
                   "step_ms_rounds": [float(x) for x in ms[p]], "device_ops_per_step": launches[p],
                   "nonfinite_blocks": nonfinite[p], "end_of_last_block": end[p]} for p in PATHS}
        out["spread_ms"] = max(out[p]["step_ms_max"] - out[p]["step_ms_min"] for p in PATHS)
        out["B_minus_A_ms"] = out["B"]["step_ms_median"] - out["A"]["step_ms_median"]
        out["B_not_slower_than_A_by_more_than_the_spread"] = bool(out["B_minus_A_ms"] <= out["spread_ms"])
        res[arch] = out
        print(f"{arch}: A {out['A']['step_ms_median']:.3f} ms, B {out['B']['step_ms_median']:.3f} ms, spread {out['spread_ms']:.3f} ms",
              file=sys.stderr)
        del model, opt
        torch.cuda.empty_cache()
    lib.rgbnm_set_option(b"f16_tuned", tuned0)
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
