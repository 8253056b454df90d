#!/usr/bin/env python
"""Time what the fp16 augment output and the longer RandAugment chains change, on one GPU, configurations interleaved:

  (a) augment   the augment launch pair at B = 256, S = 28, two ops, output float32 / bfloat16 / float16, the same drawn parameters
                for all three (float16 goes through rgbnm_dct_augment_chain, the others through rgbnm_dct_augment_ex)
  (b) step      the fp16 training step of tools/fp16_step.py's JPEG-Ti configuration (autocast(float16), library defaults:
                augment, lazy mixup, forward, loss, backward, fused optimizer) fed the float16 augment output, against the same
                step fed float32
  (c) chain4    four ops per image in ONE launch pair (TrainTransform_DCT(num_ops=4), sample_chain -> apply_packed(ops=...)),
                against the same ops as two passes of two: the first pass writes int16, the second reads it back (identity crop,
                unit tables) and writes the output -- the route a chain took when a pass held two ops.  Same output bits (checked).

Every configuration runs WARMUP calls, then ROUNDS interleaved blocks of the timed calls (order reversed every other round),
device events around each block after a synchronise.  Reported per configuration: median / min / max over the blocks' per-call
times, and per comparison the difference of the medians next to the spread (the largest max - min of the two).
Writes profiles/aug_chain.json and prints it.
usage: python tools/aug_chain_step.py [--iters 200] [--steps 120] [--warmup 30] [--rounds 6] [--batch 256]
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
from rgb_no_more_amd import custom_transforms as CT, lib as L  # noqa: E402
from bench import synth_coefficients  # noqa: E402


def timed(configs, fns, warmup, rounds, per, before=None):
    """fns[cfg](): one call.  -> cfg -> list of per-call ms, one per round."""
    for cfg in configs:
        if before:
            before(cfg)
        for _ in range(warmup):
            fns[cfg]()
    torch.cuda.synchronize()
    ms = {cfg: [] for cfg in configs}
    for r in range(rounds):
        for cfg in (configs if r % 2 == 0 else configs[::-1]):
            if before:
                before(cfg)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                fns[cfg]()
            e1.record()
            torch.cuda.synchronize()
            ms[cfg].append(e0.elapsed_time(e1) / per)
    return ms


def summary(ms):
    return {cfg: {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "ms_rounds": [float(x) for x in v]}
            for cfg, v in ms.items()}


def compare(out, a, b):
    """b against a: difference of the medians and the spread it has to be read against."""
    spread = max(out[a]["ms_max"] - out[a]["ms_min"], out[b]["ms_max"] - out[b]["ms_min"])
    d = out[b]["ms_median"] - out[a]["ms_median"]
    return {"minus": a, "of": b, "delta_ms": d, "ratio": out[b]["ms_median"] / out[a]["ms_median"], "spread_ms": spread,
            "beyond_the_spread": bool(abs(d) > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="augment calls per timed block, (a) and (c)")
    ap.add_argument("--steps", type=int, default=120, help="training steps per configuration over all rounds, (b)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_chain.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, S = a.batch, 28
    res = {"batch": B, "size": S, "iters": a.iters, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash()}
    Yq, Cq, quant = synth_coefficients(B, dev, 1234)
    DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

    # ---- (a) the augment pair per output type
    augs = {k: CT.TrainTransform_DCT(size=S, out_dtype=dt) for k, dt in DT.items()}
    packed, nops = CT.FastParamSampler(augs["f32"], seed=1234).sample(B, 64, 64)
    for t in augs.values():
        t.bank = augs["f32"].bank
    fns = {k: (lambda t=t: CT.apply_packed(t, Yq, Cq, quant, packed, nops)) for k, t in augs.items()}
    y32, _ = fns["f32"]()
    y16, _ = fns["f16"]()
    assert torch.equal(y16, y32.half())
    out = summary(timed(list(DT), fns, a.warmup, a.rounds, a.iters))
    out["f16_vs_bf16"] = compare(out, "bf16", "f16")
    out["f16_vs_f32"] = compare(out, "f32", "f16")
    res["augment"] = out
    print("augment: " + ", ".join(f"{k} {out[k]['ms_median']:.4f} ms" for k in DT), file=sys.stderr)

    # ---- (c) four ops: one launch pair against two
    t4 = CT.TrainTransform_DCT(size=S, num_ops=4, out_dtype=torch.float32)
    p4, ops4, n4 = CT.FastParamSampler(t4, seed=1234).sample_chain(B, 64, 64)
    first = CT.TrainTransform_DCT(size=S, out_dtype=torch.int16)
    second = CT.TrainTransform_DCT(size=S, out_dtype=torch.float32)
    first.bank = second.bank = t4.bank
    pa, pb = p4.copy(), np.zeros(B, dtype=CT.AUG_DTYPE)
    pb["crop"] = (0, 0, S, S)
    for f in ("op", "fmag", "iarg0", "iarg1", "iarg2"):
        pa[f], pb[f] = ops4[f][:, :2], ops4[f][:, 2:]
    unit = second._unit_quant(B, dev)

    def two_passes():
        iy, ic = CT.apply_packed(first, Yq, Cq, quant, pa, 2)
        return CT.apply_packed(second, iy, ic, unit, pb, 2)
    fns = {"one_pass": lambda: CT.apply_packed(t4, Yq, Cq, quant, p4, n4, ops=ops4), "two_passes": two_passes}
    (ay, ac), (by, bc) = fns["one_pass"](), fns["two_passes"]()
    assert torch.equal(ay, by) and torch.equal(ac, bc)
    out = summary(timed(list(fns), fns, a.warmup, a.rounds, a.iters))
    out["one_vs_two"] = compare(out, "two_passes", "one_pass")
    res["chain4"] = out
    print("chain4: " + ", ".join(f"{k} {out[k]['ms_median']:.4f} ms" for k in fns), file=sys.stderr)

    # ---- (b) the fp16 step fed f16 / f32
    torch.manual_seed(0)
    model = rg.ViT(3, 16, 192, depth=12, n_classes=1000, drop_p=0.0, device=dev, num_heads=3, head_size=64, pixel_space="DCT",
                   ver=1, use_subblock=True)
    model.train()
    opt = rg.custom_optims.FusedClipAdamWWD(model, lr=1e-3, eps=1e-8, weight_decay=1e-4, max_norm=1.0)
    lab = torch.randint(0, 999, (B,), device=dev)
    legs = {}
    for k in ("f32", "f16"):
        mix = rg.cls_transforms.RandomMixup_DCT(1000, alpha=0.2)
        mix.out_dtype = DT[k]
        mix.lazy, mix.lazy_target = True, True
        legs["fed_" + k] = (augs[k], CT.FastParamSampler(augs[k], seed=1234), mix)
    last = {}

    def step(cfg):
        aug, sampler, mix = legs[cfg]
        pk, n = sampler.sample(B, 64, 64)
        y, c = CT.apply_packed(aug, Yq, Cq, quant, pk, n)
        (my, mc), mt = mix((y, c), lab, lam=mix.sample_lambda(dev))
        with torch.autocast("cuda", dtype=torch.float16):
            logits = model(my, mc)
        loss = rg.cls_transforms.cross_entropy(logits, mt, grad_dtype=torch.float16)
        loss.backward()
        opt.step()
        last[cfg] = loss
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cfgs = list(legs)
    ms = timed(cfgs, {c: (lambda c=c: step(c)) for c in cfgs}, a.warmup, a.rounds, max(1, a.steps // a.rounds),
               before=lambda cfg: model.load_state_dict(state))        # every block from the same weights (no loss scaler here)
    out = summary(ms)
    for c in cfgs:
        out[c]["last_loss_finite"] = bool(torch.isfinite(last[c]).item())
    out["f16_vs_f32"] = compare(out, "fed_f32", "fed_f16")
    res["step_fp16_vitti"] = out
    print("step: " + ", ".join(f"{k} {out[k]['ms_median']:.4f} ms" for k in cfgs), file=sys.stderr)

    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
