#!/usr/bin/env python
"""Time the JPEG-Ti training step (depth 12, B = 256, static inputs: the data stage is outside both loops) two ways, in one
process, alternating:

  a  today's loop: a HIP graph of forward -> loss -> backward (what bench.py replays), then on the host train.py's warm-up /
     torch CosineAnnealingLR (train.py:149-152, 174-176) and FusedClipAdamWWD.step -- the tail's two launches come from Python
  b  graphstep.CapturedTrainStep.replay(): the same step with the tail inside the graph and the schedule on the device
     (custom_optims.DeviceLRSchedule, rgbnm_clip_adamw_wd_step_sched)

in two configurations: bf16 (no loss scaler), and fp16 with option f16_tuned = 1 under a DeviceLossScaler.
Both loops warm up, then run ROUNDS interleaved blocks; every block starts from the same weights, moments, state blocks and
schedule position.  Per block: device ms/step (HIP events around the block), host ms/step (host clock around the loop, before
the synchronise: what the host spends issuing a step) and wall ms/step (the same clock after the synchronise).
Loop a runs code this measurement's subject does not touch: it is the baseline.  Writes profiles/captured_step.json.
usage: python tools/captured_step.py [--steps 100] [--warmup 30] [--rounds 6]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rgb_no_more_amd as rg  # noqa: E402
from rgb_no_more_amd import lib as L  # noqa: E402
from rgb_no_more_amd.custom_optims import DeviceLossScaler, DeviceLRSchedule, FusedClipAdamWWD  # noqa: E402

LR, WD, LR_WARMUP = 1e-3, 1e-4, 20
PATHS = ("a", "b")


def measure(cdt, use_scaler, a, dev):
    B, per = a.batch, a.steps
    torch.manual_seed(0)
    model = rg.ViT(3, 16, 192, depth=12, n_classes=1000, drop_p=0.0, device=dev, num_heads=3, head_size=64, pixel_space="DCT",
                   ver=1, use_subblock=True)
    model.compute_dtype = cdt
    model.defer_grad_reduction = True           # as bench.py on one GPU
    model.train()
    model._ensure_flat()
    y = torch.randn(B, 1, 28, 28, 8, 8, device=dev)
    c = torch.randn(B, 2, 14, 14, 8, 8, device=dev)
    tgt = torch.rand(B, 1000, device=dev)
    tgt = tgt / tgt.sum(1, keepdim=True)
    w0 = model._flat.clone()

    # b: the whole step captured
    opt_b = FusedClipAdamWWD(model, lr=LR, eps=1e-8, weight_decay=WD, max_norm=1.0)
    sched = DeviceLRSchedule.warmup_cosine(LR, LR_WARMUP, per)
    scaler_b = DeviceLossScaler() if use_scaler else None
    whole = rg.CapturedTrainStep(model, opt_b, sched, loss_scaler=scaler_b).capture(y, c, tgt)
    blocks_b = whole._blocks()
    saved_b = [t.clone() for t in blocks_b]

    # a: forward -> loss -> backward captured, the tail and the scheduler on the host
    opt_a = FusedClipAdamWWD(model, lr=LR, eps=1e-8, weight_decay=WD, max_norm=1.0)
    scaler_a = DeviceLossScaler() if use_scaler else None

    def fwd_bwd():
        loss = rg.cls_transforms.cross_entropy(model(y, c), tgt, grad_dtype=cdt)
        (scaler_a.scale(loss) if use_scaler else loss).backward()
        return loss
    for _ in range(3):
        opt_a.zero_grad(set_to_none=True)
        fwd_bwd()
    (scaler_a.step(opt_a) if use_scaler else opt_a.step())        # the tail's own first use (state, uploads)
    opt_a.zero_grad(set_to_none=True)
    part = torch.cuda.CUDAGraph()
    with torch.cuda.graph(part, stream=torch.cuda.current_stream()):
        loss_a = fwd_bwd()
    saved_scaler_a = scaler_a._state.clone() if use_scaler else None

    def restart(path):
        model._flat.copy_(w0)
        if path == "b":
            for t, s in zip(blocks_b, saved_b):
                t.copy_(s)
            return None
        opt_a._exp_avg.zero_()
        opt_a._exp_avg_sq.zero_()
        if use_scaler:
            scaler_a._state.copy_(saved_scaler_a)
            scaler_a._state[2:3].zero_()          # the Adam step count lives in the block
        else:
            opt_a._step = 0
        opt_a.param_groups[0]["lr"] = LR
        opt_a.param_groups[0].pop("initial_lr", None)
        return torch.optim.lr_scheduler.CosineAnnealingLR(opt_a, T_max=per - LR_WARMUP, eta_min=0)

    def run(path, n, cos):
        if path == "b":
            for _ in range(n):
                loss = whole.replay()
            return loss
        current_itr = 0
        for _ in range(n):
            current_itr += 1
            if current_itr < LR_WARMUP:
                opt_a.param_groups[0]["lr"] = LR * (current_itr + 1) / LR_WARMUP
            part.replay()
            if use_scaler:
                scaler_a.step(opt_a)
                scaler_a.update()
            else:
                opt_a.step()
            if current_itr >= LR_WARMUP:
                cos.step()
        return loss_a

    for path in PATHS:
        cos = restart(path)
        run(path, a.warmup, cos)
    torch.cuda.synchronize()
    keys = ("device_ms", "host_ms", "wall_ms")
    t = {p: {k: [] for k in keys} for p in PATHS}
    end_w = {}
    for r in range(a.rounds):
        for path in (PATHS if r % 2 == 0 else PATHS[::-1]):
            cos = restart(path)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            e0.record()
            loss = run(path, per, cos)
            e1.record()
            h1 = time.perf_counter()
            torch.cuda.synchronize()
            h2 = time.perf_counter()
            assert bool(torch.isfinite(loss).all()), (path, r)
            t[path]["device_ms"].append(e0.elapsed_time(e1) / per)
            t[path]["host_ms"].append((h1 - h0) * 1e3 / per)
            t[path]["wall_ms"].append((h2 - h0) * 1e3 / per)
            end_w[path] = model._flat.clone()
    out = {}
    for p in PATHS:
        out[p] = {}
        for k in keys:
            v = t[p][k]
            out[p][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": [float(x) for x in v]}
    for k in keys:
        spread = max(out[p][k]["max"] - out[p][k]["min"] for p in PATHS)
        diff = out["b"][k]["median"] - out["a"][k]["median"]
        out[k + "_spread"] = spread
        out[k + "_b_minus_a"] = diff
        out[k + "_b_not_slower_than_a_beyond_the_spread"] = bool(diff <= spread)
    # the two loops end a block at the same weights (fp16: same entry arithmetic, bit for bit; bf16: loop a takes the plain entry,
    # whose host-side bias corrections may differ from the device's by one fp32 ulp)
    out["end_weights_bit_equal"] = bool(torch.equal(end_w["a"], end_w["b"]))
    out["end_weights_max_abs_diff"] = float((end_w["a"] - end_w["b"]).abs().max())
    out["schedule_iteration_after_block"] = sched.iteration()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="steps per block")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "captured_step.json"))
    ap.add_argument("--f16-tuned", type=int, default=1, choices=(1, 2), help="level of the option f16_tuned for the fp16 configuration")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.rounds >= 6 and a.steps > LR_WARMUP
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.cuda.set_stream(torch.cuda.Stream())       # one non-default stream for everything, as bench.py
    lib = L.lib()
    tuned0 = lib.rgbnm_get_option(b"f16_tuned")
    res = {"arch": "vitti", "batch": a.batch, "steps_per_block": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "source_hash": L.source_hash(), "f16_tuned": a.f16_tuned,
           "loops": {"a": "HIP graph of forward -> loss -> backward, then host warm-up / CosineAnnealingLR and FusedClipAdamWWD.step",
                     "b": "CapturedTrainStep.replay(): one HIP graph with the tail and the device schedule inside"}}
    for name, cdt, scaler, tuned in (("bf16", torch.bfloat16, False, tuned0), ("fp16_tuned_device_scaler", torch.float16, True, a.f16_tuned)):
        lib.rgbnm_set_option(b"f16_tuned", tuned)
        res[name] = measure(cdt, scaler, a, dev)
        o = res[name]
        print(f"{name}: device a {o['a']['device_ms']['median']:.3f} b {o['b']['device_ms']['median']:.3f} ms "
              f"(spread {o['device_ms_spread']:.3f}); host a {o['a']['host_ms']['median']:.3f} b {o['b']['host_ms']['median']:.3f} ms",
              file=sys.stderr)
        torch.cuda.empty_cache()
    lib.rgbnm_set_option(b"f16_tuned", tuned0)
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
